/*
 * pgo.h -- C-ABI of the MI355X-native 2D pose-graph backend (libpgo.so).
 *
 * This is the drop-in boundary for ONE path of wei-ght/toy-robust-backend-slam:
 * DCS-ceres/main.cpp METHOD 0/1 (SE(2) odometry + loop-closure least squares,
 * Dynamic Covariance Scaling, HuberLoss(0.01), Ceres LM) and, since SURVEY.md section 8(f) ranks it
 * next, METHOD 2 (switchable constraints).  Everything the
 * reference does between `ceres::Problem problem;` (main.cpp:66) and the end of
 * `ceres::Solve` (main.cpp:163) is replaced by pgo_create / pgo_solve /
 * pgo_get_poses; the g2o loader, classifier, outlier injector and writers
 * (include/g2o_util.h:23-186) are replaced by the pgo_g2o_* / pgo_inject_* /
 * pgo_write_* host functions.  All citations are relative to /root/reference/DCS-ceres.
 *
 * Conventions
 *   - plain pointers + sizes only; the caller owns every host array it passes;
 *     the library copies in at create and copies out on get.
 *   - every function returns 0 on success or a negative pgo_status.
 *     No exception crosses this boundary.
 *   - a pgo_t handle is NOT thread-safe: one handle per host thread.
 *   - functions marked [host] never touch the GPU and work on a GPU-less box;
 *     functions marked [gpu] require a gfx950 device and fail with
 *     PGO_ERR_NO_DEVICE otherwise (there is no CPU fallback on the product path).
 */
#ifndef PGO_H_
#define PGO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
typedef enum pgo_status {
  PGO_OK = 0,
  PGO_ERR_INVALID_ARG = -1,   /* null pointer, bad size, bad index            */
  PGO_ERR_IO = -2,            /* file cannot be opened / written              */
  PGO_ERR_PARSE = -3,         /* malformed g2o record                         */
  PGO_ERR_NO_DEVICE = -4,     /* no gfx950 device visible                     */
  PGO_ERR_HIP = -5,           /* a HIP runtime call failed                    */
  PGO_ERR_COMM = -6,          /* RCCL / shm communicator failure              */
  PGO_ERR_NUMERIC = -7,       /* non-finite residual/Jacobian at the current point
                                 (Ceres: "Residual and Jacobian evaluation failed") */
  PGO_ERR_UNSUPPORTED = -8,   /* METHOD 3/4 etc.                              */
  PGO_ERR_NOMEM = -9
} pgo_status;

const char* pgo_strerror(int status);           /* [host] static string           */
const char* pgo_last_error(void);               /* [host] thread-local detail text */
const char* pgo_version(void);                  /* [host]                          */

/* edge kinds: include/g2o_util.h:14-16 */
#define PGO_EDGE_ODOMETRY 0
#define PGO_EDGE_CLOSURE 1
#define PGO_EDGE_BOGUS 2

/* ------------------------------------------------------ g2o graph (host side)
 * Replaces class ReadG2O (include/g2o_util.h:20-188) + Node/Edge (include/graph.h).
 * The graph is held as flat arrays; edges are stored in the reference's
 * residual-block order: all odometry, then all closure, then all bogus
 * (main.cpp:95-150).                                                          */
typedef struct pgo_graph pgo_graph;

/* ReadG2O::ReadG2O (g2o_util.h:23-89).  Same tags (VERTEX_SE2|VERTEX2,
 * EDGE_SE2|EDGE2), same positional fields, same classifier: odometry iff
 * abs(a-b) < 5 (g2o_util.h:68), endpoints addressed by vector position
 * (g2o_util.h:70,77).  Unlike the reference, I/O and range errors are reported. */
int pgo_g2o_load(const char* path, pgo_graph** out);                       /* [host] */
/* same, from a memory buffer (used by tests and by the synthetic generator)      */
int pgo_g2o_parse(const char* text, size_t len, pgo_graph** out);          /* [host] */
/* build a graph directly from arrays (kind[] decides the three lists)            */
int pgo_graph_from_arrays(int32_t n_poses, const double* poses_xyt,
                          int32_t n_edges, const int32_t* ia, const int32_t* ib,
                          const double* meas_xyt, const double* info6_or_null,
                          const uint8_t* kind, pgo_graph** out);           /* [host] */
void pgo_graph_free(pgo_graph* g);                                         /* [host] */

int32_t pgo_graph_num_poses(const pgo_graph* g);
int32_t pgo_graph_num_edges(const pgo_graph* g);            /* odo + closure + bogus */
int32_t pgo_graph_num_edges_of_kind(const pgo_graph* g, int kind);
/* borrowed pointers, valid until the graph is mutated or freed                    */
const int32_t* pgo_graph_pose_ids(const pgo_graph* g);      /* Node::index          */
double*        pgo_graph_poses(pgo_graph* g);               /* N x 3 (x,y,theta), mutable: Node::p */
const int32_t* pgo_graph_edge_a(const pgo_graph* g);        /* position of Edge::a  */
const int32_t* pgo_graph_edge_b(const pgo_graph* g);
const double*  pgo_graph_edge_meas(const pgo_graph* g);     /* E x 3 (x,y,theta)    */
const double*  pgo_graph_edge_info(const pgo_graph* g);     /* E x 6 I11 I12 I13 I22 I23 I33 (parsed, unused: SURVEY H5) */
const uint8_t* pgo_graph_edge_kind(const pgo_graph* g);

/* ReadG2O::add_random_C (g2o_util.h:151-171): `count` bogus loops drawn with the
 * C library rand() in the reference's call order (a, b, m0, m1, m2), measurement
 * rand()/RAND_MAX in INTEGER arithmetic, info (2,0,0,300,0,300).
 * seed >= 0: srand(seed) first (reproducible);  seed < 0: srand(time(0)) as
 * main.cpp:43 does.                                                              */
int pgo_inject_outliers(pgo_graph* g, int32_t count, int64_t seed);        /* [host] */

/* writePoseGraph_nodes / writePoseGraph_edges (g2o_util.h:93-112,179-186).
 * precision <= 0 : the reference's default ostream formatting (6 significant
 * digits); precision > 0 : that many significant digits (17 round-trips).        */
int pgo_write_nodes(const pgo_graph* g, const char* path, int precision);  /* [host] */
int pgo_write_edges(const pgo_graph* g, const char* path);                 /* [host] */
/* writePoseGraph_switches (g2o_util.h:114-148): three sections, "<a> <b> <type> <prior> <switch>" per edge;
 * switches: E values in the graph's edge order (prior is 1.0 everywhere, as main.cpp:119,141)             */
int pgo_write_switches(const pgo_graph* g, const char* path, const double* switches); /* [host] */
/* g2o writer (VERTEX_SE2 / EDGE_SE2), for the synthetic configs                  */
int pgo_write_g2o(const pgo_graph* g, const char* path);                   /* [host] */

/* Synthetic Manhattan world (BASELINE configs C4/C5; the reference ships no
 * generator -- spec in SURVEY.md section 8(d)): unit steps on the integer grid of a
 * bounded square (side ~ sqrt(N/4), so cells are revisited), +-90 degree turns with
 * p=0.2, odometry noise N(0, 0.02 m / 0.01 rad), up to 3 closures per pose to earlier
 * poses (|i-j| >= 5) within 1.5 m, thinned to about edges_per_pose * N edges in total,
 * initial poses = dead-reckoned odometry, plus round(outlier_frac * #closures) bogus
 * loops with R4 semantics (uniform random endpoints, zero measurement).
 * PRNG: splitmix64(seed).                                                         */
int pgo_synth_manhattan(int32_t n_poses, double edges_per_pose, double outlier_frac,
                        uint64_t seed, pgo_graph** out);                   /* [host] */

/* ------------------------------------------------------------ solver options
 * Defaults (pgo_options_default) are the Ceres defaults the reference runs with
 * (main.cpp:154-163 sets only progress + SPARSE_NORMAL_CHOLESKY) plus the
 * constants hard-coded in the reference: Huber 0.01 (main.cpp:68), phi 0.5
 * (src/ceres_error.cpp:185), fixed pose 0 (main.cpp:153).                        */
typedef struct pgo_options {
  int32_t method;              /* 0 = plain (OdometryResidue everywhere), 1 = DCS on closure+bogus (main.cpp:112-114,135-137),
                                  2 = switchable constraints on closure+bogus (main.cpp:115-125,138-145) */
  int32_t max_iters;           /* 50   Solver::Options::max_num_iterations        */
  int32_t fixed_pose;          /* 0    position of the constant pose, -1 = none   */
  int32_t jacobi_scaling;      /* 1                                               */
  double  phi;                 /* 0.5  DCS upper bound                            */
  double  huber_delta;         /* 0.01 ; <= 0 disables the loss                   */
  double  ftol;                /* 1e-6  function_tolerance                        */
  double  gtol;                /* 1e-10 gradient_tolerance (max-norm)             */
  double  ptol;                /* 1e-8  parameter_tolerance                       */
  double  radius0;             /* 1e4   initial_trust_region_radius               */
  double  max_radius;          /* 1e16                                            */
  double  min_radius;          /* 1e-32                                           */
  double  min_relative_decrease; /* 1e-3                                          */
  double  min_lm_diagonal;     /* 1e-6                                            */
  double  max_lm_diagonal;     /* 1e32                                            */
  /* linear solver: block-Jacobi preconditioned CG on (J'J + D'D) y = J'r        */
  double  pcg_rtol;            /* stop when ||r|| <= pcg_rtol * ||b||  (1e-12: "exact" mode
                                  standing in for SPARSE_NORMAL_CHOLESKY; 0.1 = Ceres' eta for inexact steps) */
  int32_t pcg_max_iters;       /* cap per LM iteration                            */
  int32_t pcg_check_every;     /* iterations enqueued between host residual checks */
  int32_t verbose;             /* 1 = Ceres-like per-iteration table on stdout    */
  int32_t use_graphs;          /* 1 (default) = replay slices of pcg_check_every PCG iterations as a hipGraph (world == 1) */
  int32_t pcg_block_poses;     /* poses per block of the block-Jacobi preconditioner: 1 = the 3x3 pose blocks,
                                  2..32 = dense (3B x 3B) blocks of B consecutive poses (explicit inverses);
                                  0 = auto (32 for graphs of <= 8192 poses, which are launch-latency bound and
                                  chain-like, else 4) */
  int32_t halo_exchange;       /* world > 1: how the search direction reaches the other ranks each PCG iteration.
                                  0 (default) = in-place all-gather of all 3N doubles (exercised through RCCL, captured into
                                      the PCG hipGraph);
                                  1 (opt-in) = point-to-point halo exchange: every rank sends each peer only the rows that
                                      peer's off-diagonal blocks reference (one ncclSend/ncclRecv group on the solver's stream).
                                      Far fewer bytes, but the RCCL send/recv group has not yet run against a real peer:
                                      bench.py checks it against the all-gather result when it runs on several GPUs and
                                      times it only if the two agree                                                  */
  double  sc_prior_lambda;     /* 1.0  METHOD 2: weight of the switch prior sqrt(lambda)(1 - s)  (main.cpp:107)    */
  int32_t pose_ordering;       /* internal numbering of the poses (results are always in the caller's numbering):
                                  0 = the caller's, 1 = locality ordering (pgo_pose_order: segments of 64 consecutive
                                  poses reordered by reverse Cuthill-McKee on the loop edges that a neighbouring edge
                                  supports), -1 (default) = 1 when world > 1 (it shrinks every rank's halo) and on single-rank
                                  graphs of more than 65536 poses (the gathers of K1 / K2 / K3 then hit the XCD's L2), else 0 */
  int32_t info_weighting;      /* 0 (default) = the reference's objective: the information entries of an edge are parsed
                                  but unused.  1 = optional mode: every residual is whitened by
                                  its information matrix, e_w = L' e with Omega = L L', so |e_w|^2 = e' Omega e (the chi2
                                  of compute_edge_mahalanobis, src/layer_manager.cpp:230-282); Huber then acts on chi2 and
                                  METHOD 1 uses the chi2 form of DCS, s = min(1, 2 phi / (phi + chi2)), e = s e_w
                                  (differentiated through s, as the reference differentiates through psi).  Needs the
                                  information matrices (pgo_create_weighted / pgo_create_from_graph), all positive
                                  definite; METHOD 2: PGO_ERR_UNSUPPORTED                                            */
  int32_t pcg_chain_len;       /* chain preconditioner: block-Jacobi over segments of this many consecutive poses whose blocks
                                  are kept block-TRIDIAGONAL (the odometry chain inside the segment; every other edge only
                                  adds its 3x3 diagonal blocks), factorised exactly per LM iteration and applied by
                                  chunked wavefront scans.  A multiple of 4 that divides 256 (64 = the measured default)
                                  turns it on and overrides pcg_block_poses; 0 = off;
                                  -1 (default), with pcg_block_poses = 0 (auto): 64 on graphs of > 50000 poses; 256 on chain-like
                                  graphs of 512..8192 poses (few short-range non-consecutive edges); else off                 */
  int32_t halo_overlap;        /* 0 (default): exchange, then one SpMV launch, all on the solver's stream.
                                  1 (opt-in): with halo_exchange = 1, the exchange runs on a second stream while the SpMV
                                  multiplies the blocks whose columns are owned; the blocks that need halo rows follow.
                                  Checked against the plain schedule with the host-staged test communicator only: the
                                  RCCL send/recv group has not yet run against a real peer                              */
  int32_t linear_solver;       /* how (J'J + D'D) y = J'r is solved (the reference: SPARSE_NORMAL_CHOLESKY, main.cpp:154-163):
                                  1 = block-Jacobi PCG to pcg_rtol;
                                  2 = direct: the odometry chain (one edge per consecutive pose pair; block tridiagonal, factorised
                                      exactly) + every other edge as a low-rank term through the Woodbury identity -- a dense
                                      Cholesky of order 3 x (edges outside the chain) -- + iterative refinement.  One rank, no
                                      information weighting, a constant pose, every consecutive pose pair joined by an edge, at most 2047
                                      edges outside the chain, at most 65536 poses; else PGO_ERR_UNSUPPORTED;
                                  0 (default) = auto, when pcg_rtol <= 1e-8 (the "exact" mode) and pcg_block_poses / pcg_chain_len
                                      are left at auto: 2 where it applies with at most 682 edges outside the chain (INTEL,
                                      MIT, CSAIL, FR079 ...); with more (M3500, FRH: the dense Cholesky is no longer cheap) the
                                      solve starts with 1 and changes to 2 after an LM iteration whose PCG iteration count
                                      says PCG costs more than the direct solve (M3500 with DCS: yes, without: no); else 1      */
  int32_t pcg_coarse_poses;    /* second preconditioner level: an additive coarse correction on the RIGID-BODY modes (translation x, y,
                                  rotation about the centre) of aggregates of this many consecutive poses -- three unknowns per
                                  aggregate, Galerkin matrix P'(J'J + D'D)P factorised densely per LM iteration (order <= 6143).
                                  It removes the smooth long-range error that block-Jacobi cannot: M3500 METHOD 1, PCG to 1e-10:
                                  1557 -> 178 iterations with 16-pose aggregates.  Taken as given (not rounded to the one-level
                                  block: an aggregate may straddle two groups or segments).  0 = off;
                                  -1 (default) = auto, for graphs of >= 512 poses that stay on PCG while pcg_block_poses and
                                  pcg_chain_len are left at auto: on for tight solves
                                  (pcg_rtol <= 1e-3) -- 16 poses per aggregate up to 8192 poses, else 64, doubled until the
                                  coarse order fits; loose solves (the inexact mode) stay on one level unless asked.
                                  Several ranks (or PGO_FORCE_COLLECTIVES=1): only an explicit value > 0 enables it (auto stays
                                  one level there); the shard boundaries are then aligned to lcm(block or segment, this value),
                                  so that the aggregates are those of the one-rank solve.  The coarse problem is replicated on
                                  every rank (r_c rides in the all-reduce of the PCG dot products) and the PCG loop is the
                                  two-reduction one; pgo_handle_info reports the global level identically on every rank.     */
} pgo_options;

void pgo_options_default(pgo_options* o);                                  /* [host] */

/* ------------------------------------------------------------ robust losses
 * Ceres 2.x LossFunction semantics.  s = |e|^2 of one residual block: after the DCS scaling (METHOD 1) or the switch
 * (METHOD 2: s = |s_sw e|^2), and after whitening when info_weighting = 1.  The block's cost is 1/2 rho(s).  Every loss
 * below has rho'' <= 0, so Ceres' Corrector reduces to scaling the block's residual and Jacobian rows (and, METHOD 2,
 * d e / d s) by sqrt(rho'(s)).  Every loss has rho(0) = 0 and rho'(0) = 1.  DBL_MIN = 2.2250738585072014e-308.
 *
 *   type                  parameters          rho(s)                      rho'(s)                     rho''(s)
 *   PGO_LOSS_TRIVIAL      (Ceres' NULL loss)  s                           1                           0
 *   PGO_LOSS_HUBER        b = a^2             s <= b: s                   1                           0
 *                                             s >  b: 2 a sqrt(s) - b     max(DBL_MIN, a / sqrt(s))   -rho' / (2 s)
 *   PGO_LOSS_SOFTLONE     b = a^2, c = 1/b    2 b (sqrt(1 + c s) - 1)     max(DBL_MIN, 1/sqrt(1+cs))  -c rho' / (2 (1 + c s))
 *   PGO_LOSS_CAUCHY       b = a^2, c = 1/b    b log(1 + c s)              max(DBL_MIN, 1 / (1 + c s)) -c / (1 + c s)^2
 *   PGO_LOSS_ARCTAN       b = 1/a^2           a atan2(s, a)               max(DBL_MIN, 1/(1 + b s^2)) -2 b s / (1 + b s^2)^2
 *   PGO_LOSS_TUKEY        v = 1 - s/a^2       s <= a^2: a^2/3 (1 - v^3)   v^2                         -2 v / a^2
 *                                             s >  a^2: a^2/3             0                           0
 *
 * Under Tukey a block beyond a contributes a constant cost and zero residual and Jacobian rows, as in Ceres.
 * a must be finite and > 0 (Trivial ignores it).                                                                  */
typedef enum pgo_loss_type {
  PGO_LOSS_TRIVIAL = 0,
  PGO_LOSS_HUBER,
  PGO_LOSS_SOFTLONE,
  PGO_LOSS_CAUCHY,
  PGO_LOSS_ARCTAN,
  PGO_LOSS_TUKEY
} pgo_loss_type;
typedef struct pgo_loss {
  int32_t type;   /* pgo_loss_type */
  int32_t _pad;
  double  a;      /* scale */
} pgo_loss;
/* LossFunction::Evaluate: rho[0..2] = rho(s), rho'(s), rho''(s).  PGO_ERR_INVALID_ARG for a null pointer, an unknown type
 * or a bad scale.                                                                                                    */
int pgo_loss_evaluate(const pgo_loss* l, double s, double rho[3]);                /* [host] */

typedef enum pgo_termination {
  PGO_TERM_CONVERGENCE_FTOL = 1,
  PGO_TERM_CONVERGENCE_GTOL = 2,
  PGO_TERM_CONVERGENCE_PTOL = 3,
  PGO_TERM_NO_CONVERGENCE = 4,       /* max_iters reached                        */
  PGO_TERM_MIN_RADIUS = 5,
  PGO_TERM_FAILURE = 6
} pgo_termination;

typedef struct pgo_iter_record {     /* one row of Ceres' progress table          */
  int32_t iter;
  int32_t step_ok;                   /* 1 accepted, 0 rejected, -1 invalid        */
  double  cost;
  double  cost_change;
  double  gradient_max_norm;
  double  step_norm;
  double  relative_decrease;         /* tr_ratio                                  */
  double  radius;
  int32_t pcg_iters;
  int32_t _pad;
  double  pcg_rel_residual;
  double  seconds;
} pgo_iter_record;

typedef struct pgo_summary {
  int32_t termination;               /* pgo_termination                           */
  int32_t iterations;                /* LM iterations performed (successful + not) */
  int32_t successful_steps;
  int32_t total_pcg_iters;
  double  initial_cost;
  double  final_cost;
  double  seconds_total;
  double  seconds_eval;              /* residual + Jacobian kernel                */
  double  seconds_assemble;
  double  seconds_linear;
  double  seconds_candidate;
} pgo_summary;

/* ------------------------------------------------------------ communicator
 * One process per GPU.  The graph is sharded by pose-id range over the ranks of
 * a communicator; world == 1 needs no communicator (pass NULL to pgo_create).   */
typedef struct pgo_comm pgo_comm;
#define PGO_COMM_ID_BYTES 128
int  pgo_comm_unique_id(uint8_t id[PGO_COMM_ID_BYTES]);        /* [gpu] ncclGetUniqueId on rank 0; broadcast by the caller */
int  pgo_comm_create_rccl(const uint8_t id[PGO_COMM_ID_BYTES], int rank, int world, int device, pgo_comm** out); /* [gpu] */
/* host-staged shared-memory communicator: TEST backend only (several ranks on one
 * GPU, where RCCL refuses duplicate devices).  Same collectives, same results.   */
int  pgo_comm_create_shm(const char* name, int rank, int world, int device, pgo_comm** out);                     /* [gpu] */
void pgo_comm_destroy(pgo_comm* c);

/* ------------------------------------------------------------------ solver
 * pgo_create replaces main.cpp:66-68,95-153: it takes the whole graph (every
 * rank passes the same arrays) and keeps the shard of `comm`'s rank on `device`. */
typedef struct pgo_handle pgo_t;

int pgo_create(pgo_t** h, int32_t n_poses, const double* poses_xyt,
               int32_t n_edges, const int32_t* ia, const int32_t* ib,
               const double* meas_xyt, const uint8_t* kind,
               const pgo_options* opt, pgo_comm* comm_or_null, int device);       /* [gpu] */
/* same, with the edges' information matrices: info6 = E x 6 (I11 I12 I13 I22 I23 I33, the reference's Edge fields,
 * include/graph.h:41-47) or NULL.  They are used by opt->info_weighting = 1 and by pgo_edge_chi2 only.                */
int pgo_create_weighted(pgo_t** h, int32_t n_poses, const double* poses_xyt,
                        int32_t n_edges, const int32_t* ia, const int32_t* ib,
                        const double* meas_xyt, const double* info6_or_null, const uint8_t* kind,
                        const pgo_options* opt, pgo_comm* comm_or_null, int device); /* [gpu] */
/* passes the graph's information matrices along */
int pgo_create_from_graph(pgo_t** h, const pgo_graph* g, const pgo_options* opt,
                          pgo_comm* comm_or_null, int device);                    /* [gpu] */
void pgo_destroy(pgo_t* h);

/* Problem::Evaluate equivalent.  poses_or_null == NULL evaluates at the handle's
 * current poses.  r: E x 3, J: E x 18 = [d e/d P1 (3x3 row-major) | d e/d P2],
 * both in the caller's edge order.  apply_loss != 0 applies the corrector of each
 * block's loss (r <- sqrt(rho') r, J <- sqrt(rho') J) as Ceres' ResidualBlock::Evaluate
 * does.  cost = 1/2 sum rho(|e|^2), always with the losses (pgo_set_losses; by default
 * Huber(huber_delta), no loss when huber_delta <= 0).  r/J outputs need world == 1.  */
int pgo_eval(pgo_t* h, const double* poses_or_null, int apply_loss,
             double* cost, double* r_or_null, double* J_or_null);                 /* [gpu] */

/* The loss of every residual block (a pose-graph edge) by loss class.  n_classes = 1..4 losses; edge_class lists each
 * edge's class in the caller's edge order (a batch: the problems' edges concatenated).  edge_class NULL: an edge's class is
 * min(kind, n_classes - 1) -- 1 class is one loss for every block, 2 are odometry / loops, 3 follow the edge kind.
 * A new handle has one class, Huber(huber_delta), or Trivial when huber_delta <= 0; after this call huber_delta is
 * ignored.  The losses apply to every later evaluation: pgo_eval, the LM loop, the batched solve, pgo_pose_covariance.
 * pgo_edge_chi2 and the METHOD 2 switch prior have no loss.  A solve begun with pgo_lm_begin becomes stale: pgo_lm_step
 * returns PGO_ERR_INVALID_ARG until pgo_lm_begin runs again.  Several ranks: every rank passes the same arguments.
 * PGO_ERR_INVALID_ARG: an unknown type, a non-Trivial scale that is not finite or not > 0, n_classes outside 1..4, a class
 * index >= n_classes, a null pointer.                                                                                 */
int pgo_set_losses(pgo_t* h, int32_t n_classes, const pgo_loss* losses,
                   const uint8_t* edge_class_or_null);                            /* [gpu] */

/* compute_edge_mahalanobis (src/layer_manager.cpp:230-282; the layer managers' edge gate) for every edge at once:
 * chi2[e] = r' Omega r of the PLAIN residual r = (ex, ey, asin(clamp(sin delta, -1, 1))), clamped at 0, in the
 * caller's edge order, at the handle's current poses or at poses_or_null.  Independent of opt->method and
 * opt->info_weighting; any symmetric Omega.  Needs a handle created with information matrices.
 * world > 1: every rank gets the whole vector (one all-reduce).                                                */
int pgo_edge_chi2(pgo_t* h, const double* poses_or_null, double* chi2_out /* E */);   /* [gpu] */

/* ceres::Solve (main.cpp:163): LM from the current poses for opt.max_iters.      */
int pgo_solve(pgo_t* h, pgo_summary* s);                                          /* [gpu] */
/* Many independent problems at once (the reference's layer managers run ceres::Solve per candidate layer / window,
 * src/simple_layer_manager.cpp:457-622, src/layer_manager.cpp:104-179): pgo_solve on each of the n handles, driven by
 * up to max_concurrency host threads (<= 0: 8).  Every handle has its own HIP stream, so the launch-bound small solves
 * overlap on the device; each handle's result is bitwise what pgo_solve alone gives.  summaries: n entries or NULL.
 * Handles with a communicator are refused (PGO_ERR_UNSUPPORTED).  Returns the first failing status.                */
int pgo_solve_batch(pgo_t* const* handles, int32_t n, pgo_summary* summaries, int32_t max_concurrency);   /* [gpu] */
/* The batch as ONE handle (what the layer managers' evaluate_layer_cost / optimize_layer / optimize_local_window loops
 * want, src/simple_layer_manager.cpp:457-622): the block-diagonal union of n independent problems.  One launch of the
 * fused edge kernel, of the assembly kernel and of the preconditioner set-up covers every problem; each problem's linear
 * system is solved by its own workgroup in a single launch (the whole PCG solve, device-resident scalars); radius, cost,
 * accept / reject and termination are kept per problem and every problem stops by its own tests.  About ten launches per
 * LM iteration for the whole batch.  Every problem's result equals what pgo_solve gives for it alone up to the
 * association of floating-point sums.  One set of options for all problems: METHOD 0 or 1, opt->fixed_pose = the
 * constant pose of EVERY problem (its own numbering), preconditioner = chain segments (what the library would choose for
 * the largest problem alone; 64-pose segments where that would be dense pose blocks) or pcg_block_poses = 1.
 * Not supported (PGO_ERR_UNSUPPORTED): METHOD 2, info_weighting, a row with more than 256 incident edges, a communicator. */
typedef struct pgo_batch pgo_batch_t;
int pgo_batch_create(pgo_batch_t** b, int32_t n_problems, const pgo_graph* const* graphs,
                     const pgo_options* opt, int device);                          /* [gpu] */
void pgo_batch_destroy(pgo_batch_t* b);
int32_t pgo_batch_size(const pgo_batch_t* b);
/* ceres::Solve on every problem; summaries: n entries or NULL */
int pgo_batch_solve(pgo_batch_t* b, pgo_summary* summaries);                      /* [gpu] */
int pgo_batch_get_poses(pgo_batch_t* b, int32_t problem, double* out_xyt);        /* [gpu] */
int pgo_batch_set_poses(pgo_batch_t* b, int32_t problem, const double* poses_xyt); /* [gpu] */
/* pgo_set_losses for the whole batch: edge_class (or NULL) over the problems' edges concatenated in problem order */
int pgo_batch_set_losses(pgo_batch_t* b, int32_t n_classes, const pgo_loss* losses,
                         const uint8_t* edge_class_or_null);                      /* [gpu] */
int32_t pgo_batch_num_iter_records(const pgo_batch_t* b, int32_t problem);
int pgo_batch_get_iter_records(const pgo_batch_t* b, int32_t problem, pgo_iter_record* out, int32_t cap);

/* ------------------------------------------------------------ active sets
 * Which residual blocks (edges) and which parameter blocks (poses) the handle's problem has, from now on -- the layer
 * managers' many ceres::Solve calls over subsets of the loop edges and over windows of poses of the SAME graph
 * (src/simple_layer_manager.cpp:457-622, src/layer_manager.cpp:104-179,602-654) without a new handle per call.
 *   edge_active   E bytes in the caller's edge order, non-zero = the edge is a residual block; NULL = all.
 *   pose_constant N bytes in the caller's pose order, non-zero = SetParameterBlockConstant; NULL = none.
 * Batch: the arrays are the problems' edges / poses concatenated in problem order, like pgo_batch_set_losses.
 * - An inactive edge is not in the problem: it adds nothing to the cost, the gradient, J'J, the Jacobi scale or the DCS /
 *   loss bookkeeping; its rows in pgo_eval's r / J outputs are exactly 0; a non-finite residual or Jacobian of it is NOT an
 *   evaluation failure (a candidate loop at |sin delta| = 1 does not poison a solve that does not use it).  pgo_edge_chi2
 *   ignores the mask: it is the gate that decides what to activate.
 * - Resolved constant set = {opt.fixed_pose if >= 0} + pose_constant + every pose with no active edge (a parameter block Ceres
 *   would not have in the problem: it neither makes the system singular nor counts as "a pose without edges").  Constant
 *   poses never move (bitwise).  An active edge between two constant poses still counts in the cost (Ceres' fixed_cost).
 * - Gauge: pose_constant alone may anchor a window that does not contain opt.fixed_pose; a problem left without an anchor is
 *   the caller's business, exactly as fixed_pose = -1 is.
 * - A solve begun with pgo_lm_begin becomes stale, as after pgo_set_losses: pgo_lm_step returns PGO_ERR_INVALID_ARG until
 *   pgo_lm_begin runs again.  The poses are kept.
 * - pgo_set_losses / pgo_batch_set_losses leave the active set as it is, in either order of the calls.
 * - pgo_set_active(h, NULL, NULL) restores the handle completely: a pgo_solve after it gives bitwise what a fresh handle gives.
 * - The direct solve (linear_solver 2) stays in force while every edge of its odometry chain is active (inactive loop edges
 *   are zero columns of the low-rank term); while a chain edge is inactive the handle solves by PCG and pgo_handle_info says
 *   linear_solver 1.  pgo_pose_covariance works on the active problem: resolved-constant poses have zero blocks.
 * - Errors: PGO_ERR_UNSUPPORTED for METHOD 2, a communicator or PGO_FORCE_COLLECTIVES=1; PGO_ERR_INVALID_ARG for a null
 *   handle.  Nothing changes on error.                                                                              */
int pgo_set_active(pgo_t* h, const uint8_t* edge_active_or_null, const uint8_t* pose_constant_or_null);             /* [gpu] */
int pgo_batch_set_active(pgo_batch_t* b, const uint8_t* edge_active_or_null, const uint8_t* pose_constant_or_null); /* [gpu] */
/* the resolved sets, pure logic (what the two calls above apply): constant_out[i] != 0 for the resolved constant poses */
int pgo_active_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib,
                    const uint8_t* edge_active_or_null, const uint8_t* pose_constant_or_null, int32_t fixed_pose,
                    uint8_t* constant_out /* N */, int32_t* n_active_edges, int32_t* n_free_poses);             /* [host] */

/* the same minimiser, resumable: (re)start with pgo_lm_begin, then run LM
 * iterations in slices (bench.py times slices); returns *done != 0 once a
 * termination test fired.                                                        */
int pgo_lm_begin(pgo_t* h);                                                       /* [gpu] */
int pgo_lm_step(pgo_t* h, int32_t n_iters, int32_t* done, pgo_summary* s);        /* [gpu] */
int32_t pgo_num_iter_records(const pgo_t* h);
int pgo_get_iter_records(const pgo_t* h, pgo_iter_record* out, int32_t cap);

/* What the handle resolved its "auto" options to and the size of its shard (bench.py / reports read this instead of
 * repeating the library's rules).                                                                                   */
typedef struct pgo_handle_info {
  int32_t n_poses, n_edges;          /* the whole graph                                                             */
  int32_t world, rank;
  int32_t row_lo, row_hi;            /* owned rows, internal numbering                                              */
  int32_t n_edges_local;             /* edges touching an owned row                                                 */
  int32_t n_tiles;                   /* row tiles of K2 / K3                                                        */
  int64_t n_incidences;              /* off-diagonal blocks of the owned rows                                       */
  int32_t pcg_block_poses;           /* resolved: poses per dense preconditioner block (1 when the chain form is on) */
  int32_t pcg_chain_len;             /* resolved: segment length of the chain preconditioner, 0 = off               */
  int32_t chain_kernel;              /* 2 / 4 = poses per lane of the chain apply kernels (0 without the chain form)*/
  int32_t pose_ordering;             /* resolved: 1 = internal locality ordering in use                             */
  int32_t halo_exchange;             /* resolved: 1 = point-to-point halo exchange, 0 = all-gather / single rank    */
  int32_t halo_overlap;              /* resolved                                                                    */
  int64_t halo_send_rows, halo_recv_rows;
  int64_t device_bytes;              /* HBM allocated by the handle                                                 */
  double  host_enqueue_us_per_pcg_iter; /* host time spent in launch calls per enqueued PCG iteration so far (no waiting);
                                        with graph replay ~0, eager multi-rank loops: launches + collective calls          */
  int32_t pcg_graph_replay;          /* 1 = the PCG slices are replayed from a captured hipGraph                    */
  int32_t linear_solver;             /* resolved: 1 = PCG, 2 = direct (chain + low rank)                            */
  int32_t direct_rank;               /* order of the direct solve's dense capacitance matrix (3 x edges outside the chain) */
  int32_t direct_fallbacks;          /* LM iterations whose direct solve gave no usable step and were redone by PCG  */
  int32_t direct_switched_at;        /* auto, rank above 2048: the LM iteration after which the direct solve took over from PCG
                                        (its PCG solve cost more than a direct solve of this rank does), 0 = it has not       */
  int32_t pcg_coarse_poses;          /* resolved: poses per aggregate of the second preconditioner level, 0 = one level   */
  int32_t pcg_coarse_rank;           /* order of its dense coarse matrix (all aggregates of the graph; the same on every rank) */
  int32_t pcg_single_reduction;      /* 1 = the PCG loop with ONE reduction point per iteration (Chronopoulos-Gear recurrences:
                                        world > 1, pcg_rtol >= 1e-6, chain preconditioner), 0 = the textbook two-reduction loop */
  int32_t pcg_coarse_off_iters;      /* LM iterations whose PCG solve ran WITHOUT the second level because its factorisation was
                                        not usable (a pivot lost to rounding); 0 on a healthy solve                          */
  int32_t direct_separators;         /* direct solve: separator poses the chain is cut at (0 below 256 poses)              */
  int32_t direct_segments;           /* direct solve: segments of the chain sweeps (32, fewer on chains shorter than that)   */
  int32_t direct_refine_kernel;      /* direct solve: the refinement's column is solved by 1 = k_dlr_solve1 (one launch, up to
                                        4096 poses), 2 = the batched sweep kernels; 0 = not on the direct solve             */
  int32_t n_active_edges;            /* resolved (pgo_set_active): residual blocks of the handle's problem                   */
  int32_t n_constant_poses;          /* resolved: constant poses -- opt.fixed_pose, pose_constant, poses without an active edge */
} pgo_handle_info;
int pgo_get_info(const pgo_t* h, pgo_handle_info* out);                           /* [host] */

int pgo_get_poses(pgo_t* h, double* out_xyt /* N x 3 */);                         /* [gpu] */
/* METHOD 2: current switch per edge in the caller's edge order (1.0 for odometry edges); optionally also
 * d e / d s (E x 3, after the loss corrector) of the latest Jacobian evaluation.  world == 1.              */
int pgo_get_switches(pgo_t* h, double* switches /* E */, double* js_or_null /* E x 3 */);   /* [gpu] */
int pgo_set_poses(pgo_t* h, const double* poses_xyt);                             /* [gpu] */

/* ------------------------------------------------------- pose covariances
 * ceres::Covariance with a constant parameter block: Sigma = (J'J)^-1 at the handle's CURRENT poses, J the Jacobian of the LM
 * loop (the corrector of each block's loss, pgo_set_losses; DCS scaling; no LM diagonal).  The constant pose has zero blocks.
 * Blocks are row-major 3x3 in (x, y, theta), symmetric: Sigma_ab is stored as 1/2 (Sigma_ab + Sigma_ba').  METHOD 2: the pose
 * marginal of the joint (poses, switches) system, at the switches of the latest LM iteration (needs pgo_lm_begin / pgo_solve).
 * Solved by PCG on the Jacobi-scaled undamped normal equations, 3 x poses_per_pass right-hand sides per pass, with the
 * handle's preconditioner set up for D'D = 0, plus the rigid-body coarse level on graphs of >= 512 poses (built at the first
 * call where the handle has none; the LM loop keeps running without it).  A column stops when its TRUE residual
 * ||S e - A x|| <= rtol ||S e||: where the PCG recurrence drifts from it, the column restarts from x with the true residual
 * while that lowers it; a true residual that stops falling above rtol is accepted up to 1e-5 (the double-precision floor
 * of an ill-conditioned system, reported in max_rel_residual), above that it is PGO_ERR_NUMERIC.  The LM state is left as
 * it was: pgo_lm_step afterwards gives bitwise the records and poses it gives without the call.
 * Errors: PGO_ERR_UNSUPPORTED for world > 1, no constant pose (fixed_pose = -1 and none set by pgo_set_active), info_weighting = 1 and batched
 * handles; PGO_ERR_INVALID_ARG for a bad index or a null pointer (duplicate indices are allowed); PGO_ERR_NUMERIC for a
 * non-finite pose or Jacobian, a pose without edges, a PCG breakdown, a stalled true residual or max_iters reached
 * (pgo_last_error names the pose).                                                                                       */
typedef struct pgo_covariance_options {
  double  rtol;             /* 1e-10: per column, TRUE residual ||b - A x|| <= rtol ||b||                              */
  int32_t max_iters;        /* 20000: PCG iterations per pass before PGO_ERR_NUMERIC                                   */
  int32_t poses_per_pass;   /* 8: columns per pass = 3 x this (1..16)                                                  */
  int32_t cross;            /* 0: out = n x 9 diagonal blocks; 1: out = the (3n x 3n) matrix of all blocks, row-major  */
  int32_t solver;           /* 0: PCG, as described above; 1: the handle's direct solve (below); else PGO_ERR_INVALID_ARG */
} pgo_covariance_options;
/* solver = 1 (pgo_pose_covariance and pgo_edge_gate alike) solves the same system A X = B with the factorisation a handle on the
 * direct solve owns (pgo_handle_info.linear_solver == 2: chain + low rank, set up once per call at D'D = 0), up to 768 columns
 * per pass -- the library's choice, fewer where the panels of a pass would exceed 512 MiB; poses_per_pass and max_iters are not
 * read -- and iterative refinement against A: one step always, then the TRUE residual of every column; a column above rtol
 * takes up to three more steps while the last one lowered its residual by 10 % or more; acceptance up to 1e-5 as above.
 * Results, symmetrisation, status-1 candidates, constant endpoints, `cross`, report.columns, "the LM state is left as it was"
 * and "two calls are bitwise equal" are those of solver = 0; a column's result is bitwise the same for every pass width
 * and every place in a pass.  report.passes counts the direct passes, pcg_iters_max = pcg_iters_total = 0.
 * PGO_ERR_UNSUPPORTED where the handle is not on the direct solve at the call (a PCG handle; a pgo_set_active mask that cuts
 * the odometry chain, until pgo_set_active(h, NULL, NULL)) -- never a silent fallback to PCG -- besides the refusals above.
 * PGO_ERR_NUMERIC names the pose or candidate whose residual stays above 1e-5 or is not finite: the odometry chain alone must
 * be non-singular for this path (an odometry edge whose rows a redescending loss has zeroed makes it singular where J'J is
 * not); solver = 0 still applies then.                                                                                   */
typedef struct pgo_covariance_report {
  int32_t columns, passes, pcg_iters_max, pcg_iters_total;
  double  max_rel_residual;  /* max over columns of the TRUE ||S e - A x|| / ||S e|| (<= max(rtol, floor) on success)      */
  double  seconds;
} pgo_covariance_report;
void pgo_covariance_options_default(pgo_covariance_options* o);                            /* [host] */
int  pgo_pose_covariance(pgo_t* h, int32_t n, const int32_t* poses /* caller's numbering */,
                         const pgo_covariance_options* opt_or_null, double* out,
                         pgo_covariance_report* report_or_null);                           /* [gpu]  */

/* ---------------------------------------------------- posterior sampling
 * How uncertain is EVERY pose?  pgo_pose_covariance costs three solves per pose; this call draws samples of the Gaussian
 * posterior N(0, (J'J)^-1) of the increments around the handle's CURRENT poses by perturb-and-MAP, one solve per sample:
 *   eps ~ N(0, I) in residual space (one triple per edge, one per pose prior),   (J'J) delta = J' eps   (+ R eps_p, R R' = rho' Lambda)
 * so that cov(delta) = H^-1 J'J H^-1 = H^-1 exactly.  J is what pgo_pose_covariance uses: K1's records as the last
 * linearisation left them (loss correctors, DCS, the edge weight plane, the mixtures' selected means, the active mask), on the
 * same undamped Jacobi-scaled system, through the same session: solver = 0 multi-column PCG with per-column stopping on the TRUE
 * residual, solver = 1 the handle's direct solve with refinement (768 columns a pass at most, never a fallback).
 *   delta_out   n_samples x N x 3, the caller's numbering: increments (x, y, theta) of sample first_sample + s; zero on constant poses
 *   cov_out     N x 9: (1 / n_samples) sum_s delta_s delta_s' per pose, row-major symmetric 3x3 blocks.  It is the second moment
 *               about the KNOWN mean 0 (divisor n_samples, not n_samples - 1); the whitened block is Wishart(n_samples, I) /
 *               n_samples, so its relative error depends on n_samples only: E || L^-1 C L^-T - I ||_F^2 = 12 / n_samples.
 * The noise is a pure function of (seed, stream, index, sample) -- Philox4x32-10 with key = seed and counter = (index, word,
 * sample, stream), Box-Muller on 53-bit uniforms (csrc/sample.h; pgo_sample_noise_eval evaluates it on the host): stream 0 =
 * edges, index = the edge's index in the CALLER's edge order; stream 1 = priors, index = the prior's position in the order
 * given to pgo_set_priors; sample = the global sample number.  So an edge's noise does not depend on the internal ordering, the
 * pass width or the other samples of a call, duplicate edges get independent noise, and draws compose: two calls over
 * [0, k) and [k, n) return bitwise the deltas of one call over [0, n).  Samples are summed in global sample order: cov_out is
 * bitwise independent of the pass width and of whether delta_out is asked for.  The LM state is left as it was.
 * report.columns = n_samples; the other fields as pgo_pose_covariance.
 * Errors: PGO_ERR_UNSUPPORTED as pgo_pose_covariance (world > 1, batched handles, info_weighting = 1, no constant pose, solver = 1
 * on a handle that is not on the direct solve) and for METHOD 2 (its pose marginal needs noise on the switch rows: left out);
 * PGO_ERR_INVALID_ARG for n_samples < 1, samples_per_pass outside 1..48, first_sample < 0, both outputs NULL, every pose constant;
 * PGO_ERR_NUMERIC as pgo_pose_covariance (a non-finite pose is named, a pose without edges, a stalled residual: "sample k"). */
typedef struct pgo_sample_options {
  double   rtol;             /* 1e-10, as pgo_covariance_options: TRUE residual per sample                         */
  int32_t  max_iters;        /* 20000                                                                              */
  int32_t  samples_per_pass; /* 24 (1 .. 48); solver = 1: the library's choice, not read                           */
  int32_t  solver;           /* 0 PCG, 1 the handle's direct solve (never a fallback)                              */
  int32_t  first_sample;     /* 0: this call draws samples first_sample .. first_sample + n - 1 of the seed's stream */
  uint64_t seed;
} pgo_sample_options;
void pgo_sample_options_default(pgo_sample_options* o);                                                     /* [host] */
/* the standard normal triple of (seed, stream 0 | 1, index in 0 .. 2^32 - 1, sample >= 0); else PGO_ERR_INVALID_ARG */
int  pgo_sample_noise_eval(uint64_t seed, int32_t stream, int64_t index, int32_t sample, double z[3]);      /* [host] */
int  pgo_posterior_sample(pgo_t* h, int32_t n_samples, const pgo_sample_options* opt_or_null,
                          double* delta_out_or_null /* n x N x 3, caller's numbering, (x, y, theta) increments */,
                          double* cov_out_or_null   /* N x 9 */, pgo_covariance_report* report_or_null);   /* [gpu]  */
/* test hook: the noise and the right-hand side of ONE sample.  eps_out (or NULL): E x 3 in the caller's edge order (inactive
 * edges included: their noise exists and is not used); b_out (or NULL): N x 3 in the caller's numbering, UNSCALED: J' eps
 * (+ R eps_p) on the free poses, 0 on the constant ones.  Refusals as pgo_posterior_sample.                            */
int  pgo_debug_sample_rhs(pgo_t* h, uint64_t seed, int32_t sample, double* eps_out /* E x 3, caller's edge order */,
                          double* b_out /* N x 3, caller's numbering, UNSCALED: J' eps (+ R eps_p) */);     /* [gpu]  */

/* ------------------------------------------------------------- edge gate
 * Is a candidate loop edge consistent with the current estimate, and what would it add?  For candidate k = (a, b, meas, Omega)
 * in the caller's pose numbering -- it need NOT be an edge of the graph -- at the handle's CURRENT poses:
 *   r             the plain residual (ex, ey, asin(clamp(sin delta))) of pgo_edge_chi2
 *   J             3x6 row-major [d r/d Pa | d r/d Pb] of the plain (METHOD 0) functor, with g = cos delta / sqrt(1 - sin^2 delta);
 *                 no loss and no DCS on the candidate
 *   P             J Sigma_[ab] J' (3x3 row-major, stored symmetric as 1/2 (P + P')), Sigma what pgo_pose_covariance defines on the
 *                 active problem: the covariance of the predicted residual
 *   chi2          r' Omega r, clamped at 0 (the point gate, pgo_edge_chi2)
 *   chi2_marginal r' (P + Omega^-1)^-1 r, computed as (L'r)' M^-1 (L'r) with Omega = L L', M = I + L' P L (the innovation gate)
 *   info_gain     1/2 logdet M = 1/2 logdet(I + Omega P) = 1/2 [logdet(Lambda + J' Omega J) - logdet Lambda], Lambda = J'J of the
 *                 problem.  The layer managers' 1/2 logdet(I + Omega) (src/layer_manager.cpp:284-298) is its P = I case.
 * info6 = n x 6 (I11 I12 I13 I22 I23 I33) or NULL = the identity, the weight the handle's default objective
 * (info_weighting = 0) gives every block.  The numbers are meant for edges that are NOT residual blocks of the active problem; for
 * an edge that is one they are still the quantities defined above.
 * Solved as A X = S J' on the system of pgo_pose_covariance: THREE columns per candidate (six non-zeros each), `poses_per_pass`
 * candidates per pass (1..16; the "cov_poses_per_pass" knob applies), `cross` ignored; P, the 3x3 algebra and the result
 * records are formed on the device in fixed order: two calls are bitwise equal.  Tolerance, residual replacement,
 * PGO_ERR_NUMERIC and "the LM state is left as it was" are those of pgo_pose_covariance.  report.columns counts the columns
 * solved: 3 x (candidates with status 0 and a non-zero right-hand side).
 * - A candidate whose r or J is not finite at the current poses (|sin delta| = 1) is not a call failure: status = 1, every
 *   double of its record NaN, no columns.
 * - A resolved-constant endpoint (opt.fixed_pose, pose_constant, a pose without an active edge) contributes nothing.  Both
 *   endpoints constant: P = 0 and info_gain = 0 exactly, chi2_marginal = chi2 up to rounding (the same code path), no columns.
 * Errors: PGO_ERR_UNSUPPORTED as pgo_pose_covariance (world > 1, batched handles, info_weighting = 1, no constant pose);
 * PGO_ERR_INVALID_ARG for a == b, an index out of range, an Omega that is not finite and positive definite (checked on the
 * host before any launch), a null pointer with n > 0, METHOD 2 before pgo_lm_begin.  n == 0 is PGO_OK.                   */
typedef struct pgo_edge_gate_result {
  double r[3], J[18], P[9];
  double chi2, chi2_marginal, info_gain;
  int32_t status;   /* 0 ok; 1 = non-finite r or J at the current poses: every double above is NaN */
  int32_t _pad;
} pgo_edge_gate_result;
/* the 3x3 algebra alone (csrc/gate.h, what the device runs): out = {chi2, chi2_marginal, info_gain} from r, P (row-major,
 * symmetric) and Omega.  PGO_ERR_INVALID_ARG: a null pointer, an Omega that is not finite and positive definite;
 * PGO_ERR_NUMERIC: M = I + L' P L is not positive definite (an indefinite P).                                          */
int pgo_gate_evaluate(const double r[3], const double P[9], const double* info6_or_null, double out[3]);   /* [host] */
int pgo_edge_gate(pgo_t* h, int32_t n, const int32_t* ia, const int32_t* ib, const double* meas_xyt /* n x 3 */,
                  const double* info6_or_null /* n x 6 */, const pgo_covariance_options* opt_or_null,
                  pgo_edge_gate_result* out /* n */, pgo_covariance_report* report_or_null);                /* [gpu]  */

/* ------------------------------------------------------- joint edge gate
 * pgo_edge_gate judges every candidate on its own.  The layer managers judge theirs ONE AFTER THE OTHER, each on the estimate
 * that already holds the edges accepted before it (SimpleLayerManagerV2::run, src/simple_layer_manager.cpp:74-126;
 * should_split_layer, :173-211).  pgo_edge_gate_joint gives that sequential answer, linearised at the handle's CURRENT poses,
 * from ONE covariance solve: with P = [J_j Sigma J_k'] the joint covariance of the predicted residuals of all n candidates
 * (order 3n; Sigma, r_k, J_k as pgo_edge_gate defines them) and Omega_k = L_k L_k', the working state M <- P, rho <- r is
 * walked in the CALLER'S ORDER, k = 0 .. n-1:
 *   1. r_cond = rho_k, P_cond = M_kk; chi2_cond = rho_k' (M_kk + Omega_k^-1)^-1 rho_k and info_gain_cond =
 *      1/2 logdet(I + Omega_k M_kk): pgo_gate_evaluate(rho_k, M_kk, Omega_k), the same statement (csrc/gate.h).
 *   2. accepted = status 0 and (force[k] == 1, or force[k] == -1 and chi2_cond <= chi2_gate and info_gain_cond >=
 *      min_info_gain).  force[k] == 0 rejects; force == NULL is -1 everywhere; a status-1 candidate is never accepted.
 *   3. an accepted candidate conditions the rest on it (Gaussian conditioning, a block Cholesky step of P + Omega^-1 with a
 *      3x3 pivot): C C' = I + L_k' M_kk L_k, y = C^-1 L_k' rho_k, and for i, j > k with B_i = M_ik L_k C^-T:
 *      rho_i <- rho_i - B_i y, M_ij <- M_ij - B_i B_j'.  A rejected candidate changes nothing.
 * Over the accepted set A the sums obey the chain rule: chi2_joint = r_A' (P_AA + Omega_A^-1)^-1 r_A, info_gain_joint =
 * 1/2 logdet(I + Omega_A P_AA); with every candidate forced in both are independent of the order.  After A is accepted,
 * M_kk = J_k (Lambda + sum_A J_a' Omega_a J_a)^-1 J_k' and rho_k = r_k + J_k delta, delta the Gauss-Newton step of the problem
 * augmented by A: with Omega = I and the Trivial loss that is what pgo_edge_gate returns after pgo_set_active has made the
 * edges of A residual blocks, at the same poses.  should_split_layer's question -- are the new edge and those already added
 * mutually consistent -- is this call with force = 1 on the edges already added and -1 on the new one.
 * - out[k] is bitwise what pgo_edge_gate returns for the same arguments and options (the same code path and pass plan).
 * - P_full (3n x 3n row-major, or NULL) is P, stored symmetric as 1/2 (C + C'); its diagonal blocks are bitwise out[k].P.  The
 *   rows and columns of a status-1 candidate and of one between two constant poses are exactly 0.  The blocks between candidates
 *   of different passes are formed from the solved columns after every pass (six-term gathers): no further solve.
 * - A candidate between two constant poses keeps P_cond = 0 and info_gain_cond = 0 exactly, chi2_cond = chi2 up to rounding;
 *   accepted, it alters nothing.  A status-1 candidate: every double of its joint record NaN, accepted = 0.
 * - chi2_joint and info_gain_joint: the sums of the accepted candidates' conditional numbers, in candidate order.
 * - The elimination runs on the device in fixed order, without atomics: two calls are bitwise equal.  Duplicates are allowed
 *   (Omega^-1 keeps every pivot positive definite).
 * - solver = 0 / 1, the tolerance, report, "the LM state is left as it was": those of pgo_edge_gate.
 * Errors: those of pgo_edge_gate; n > PGO_GATE_JOINT_MAX: PGO_ERR_UNSUPPORTED (split the set, or use pgo_edge_gate); a force
 * entry outside {-1, 0, 1}, a chi2_gate or min_info_gain that is NaN: PGO_ERR_INVALID_ARG; a pivot I + L' M_kk L that is not
 * positive definite: PGO_ERR_NUMERIC, pgo_last_error names the candidate.  n == 0 is PGO_OK with a zero summary.
 * pgo_gate_joint_evaluate is the elimination alone on the host (the same statements, serial): r (3n), P (3n x 3n, read as
 * given), status (n, 0 / 1) or NULL = all 0; it needs no GPU.                                                             */
#define PGO_GATE_JOINT_MAX 256          /* candidates per call: P is of order <= 768, one pass of the direct solve */
typedef struct pgo_gate_joint_options {
  double chi2_gate;       /* 7.814727903251179 (chi-square, 3 dof, 0.95); +inf = no chi2 test */
  double min_info_gain;   /* 0 */
} pgo_gate_joint_options;
typedef struct pgo_gate_joint_result {
  double r_cond[3], P_cond[9];          /* rho_k and M_kk at the moment candidate k is decided; P_cond symmetric */
  double chi2_cond, info_gain_cond;
  int32_t accepted, status;             /* status as pgo_edge_gate_result: 1 = every double NaN, accepted = 0 */
} pgo_gate_joint_result;
typedef struct pgo_gate_joint_summary { int32_t n_accepted, _pad; double chi2_joint, info_gain_joint; } pgo_gate_joint_summary;
void pgo_gate_joint_options_default(pgo_gate_joint_options*);                                   /* [host] */
int  pgo_gate_joint_evaluate(int32_t n, const double* r /*3n*/, const double* P /*3n x 3n row-major, symmetric*/,
                             const double* info6_or_null, const int32_t* status_or_null, const int8_t* force_or_null,
                             const pgo_gate_joint_options* opt_or_null,
                             pgo_gate_joint_result* joint, pgo_gate_joint_summary* sum);        /* [host] */
int  pgo_edge_gate_joint(pgo_t* h, int32_t n, const int32_t* ia, const int32_t* ib, const double* meas_xyt,
                         const double* info6_or_null, const int8_t* force_or_null,
                         const pgo_gate_joint_options* jopt_or_null, const pgo_covariance_options* opt_or_null,
                         pgo_edge_gate_result* out /* n: the independent records */, pgo_gate_joint_result* joint /* n */,
                         double* P_full_or_null /* 3n x 3n */, pgo_gate_joint_summary* sum,
                         pgo_covariance_report* report_or_null);                                /* [gpu] */

/* ---------------------------------------------------------- window solves
 * The layer managers' most frequent ceres::Solve: the local window around a newly added loop edge
 * (SimpleLayerManagerV2::optimize_local_window, src/simple_layer_manager.cpp:500-565, window_size 20 at :222,243;
 * SimpleLayerManager::optimize_layer_local, src/layer_manager.cpp:137-179) -- 42 poses, 41 edges, one constant pose, 1-2 LM
 * iterations, exact linear solve.  pgo_window_solve solves MANY such windows of the handle's graph in ONE kernel launch, one
 * workgroup per window, the whole LM loop on the device (evaluate, assemble, dense Cholesky, candidate, accept / reject,
 * termination tests); no host round trip inside the call beyond the final copy-out.
 * - Window w is the problem whose parameter blocks are the poses pose_idx[pose_ptr[w] .. pose_ptr[w+1]) and whose residual blocks
 *   are the handle's edges edge_idx[edge_ptr[w] .. edge_ptr[w+1]) (pose_ptr[0] = edge_ptr[0] = 0).  Pose indices: the caller's
 *   numbering, distinct within a window.  Edge indices: the caller's edge order (an edge may be listed twice: two residual
 *   blocks); both endpoints of every edge must be in the window's pose list.  anchor[w] is a pose of the list: the one constant
 *   block.  A listed pose without a listed edge is not in the problem (Ceres would not have it) and comes back unchanged.
 *   The handle's own active set (pgo_set_active), opt.fixed_pose and pose_constant play no part: the lists ARE the problem,
 *   as pgo_edge_gate's candidates need not be edges of the active problem.
 * - Objective and policy are the handle's: opt.method 0 or 1 (DCS on the edges whose kind says so), phi, the loss classes
 *   (pgo_set_losses; Huber(huber_delta) by default), jacobi_scaling and every LM constant of pgo_options; max_iters is the
 *   call's own, 1..PGO_WINDOW_MAX_ITERS.  The policy is that of pgo_batch_solve / pgo_solve: Jacobi scales from the initial point
 *   only; D'D = clip(diag, min_lm_diagonal, max_lm_diagonal) / radius; model decrease without the D term; the parameter and
 *   function tolerance tests on the candidate before the accept test; the same radius, decrease-factor and five-invalid-steps
 *   rules; a non-finite evaluation at the initial or at an accepted point is PGO_TERM_FAILURE.  The linear system
 *   (S J'J S + D'D) y = S J'r is solved by a dense Cholesky (what SPARSE_NORMAL_CHOLESKY is at this size): a lost pivot, a
 *   non-finite value or a non-positive model decrease is an invalid step.
 * - Every window reads the handle's CURRENT poses as they are at the call; windows are independent.  poses_out (or NULL) gets
 *   each window's final poses in list order.  commit != 0: they are also written into the handle, as pgo_set_poses would write
 *   them (a solve begun with pgo_lm_begin becomes stale); the pose lists of the call must then be pairwise disjoint (checked on
 *   the host before any launch).  commit == 0: the handle is left exactly as it was -- a following pgo_lm_step gives bitwise
 *   the records and poses it gives without the call.
 * - records (or NULL): (max_iters + 1) rows per window as the batch writes them -- row 0 the initial point, pcg_iters 0,
 *   seconds 0 --, results[w].n_records of them filled, the rest zero.
 * - No floating-point atomics; every sum runs in the order of the window's own edge and pose lists, not in the handle's internal
 *   numbering: two calls are bitwise equal, a handle with pose_ordering 1 gives bitwise what one with 0 gives, a batch gives
 *   bitwise what a solo handle with the same poses gives.
 * - A window that fails (PGO_TERM_FAILURE) is not a call failure: its poses come back unchanged, the others are unaffected.
 * - Errors: PGO_ERR_UNSUPPORTED for METHOD 2, info_weighting = 1, a communicator or PGO_FORCE_COLLECTIVES=1, a window of more
 *   than PGO_WINDOW_MAX_POSES poses or PGO_WINDOW_MAX_EDGES edges (pgo_last_error names the window; such windows stay on
 *   pgo_set_active); PGO_ERR_INVALID_ARG for a null pointer, an index out of range, a duplicate pose in a list, an edge endpoint
 *   or an anchor not in the list, max_iters out of range, overlapping lists under commit.  n_windows == 0 is PGO_OK.  Nothing
 *   changes on error.
 * pgo_batch_window_solve: the same on the problems of a batch; window w belongs to problem[w] and its indices are that
 * problem's own.                                                                                                         */
#define PGO_WINDOW_MAX_POSES 64    /* 192 unknowns: the packed triangle and the vectors take 156,032 of a workgroup's 163,840 LDS bytes */
#define PGO_WINDOW_MAX_EDGES 256   /* one lane per edge */
#define PGO_WINDOW_MAX_ITERS 32
typedef struct pgo_window_result {
  int32_t termination;        /* pgo_termination */
  int32_t iterations, successful_steps, n_records;
  double  initial_cost, final_cost;
} pgo_window_result;
/* The reference's window rule (src/simple_layer_manager.cpp:510-555), pure logic.  active = the union over the focus edges of
 * [a - radius, a + radius] and [b - radius, b + radius], clipped to [0, n_poses - 1]; edges = every PGO_EDGE_ODOMETRY edge
 * with both ends active, in graph order, followed by the focus edges with a != b in the order given, an edge listed once;
 * poses = the endpoints of those edges, ascending; anchor = pose 0 if it is among them, else the smallest (-1: no pose).  The
 * caller passes radius = max(1, window_size / 2).  A cap that is too small: the counts are still returned, the lists are not
 * written, PGO_ERR_INVALID_ARG.                                                                                           */
int pgo_window_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const uint8_t* kind,
                    int32_t n_focus, const int32_t* focus_edges, int32_t radius,
                    int32_t pose_cap, int32_t* pose_idx_out, int32_t* n_poses_out,
                    int32_t edge_cap, int32_t* edge_idx_out, int32_t* n_edges_out, int32_t* anchor_out);          /* [host] */
int pgo_window_solve(pgo_t* h, int32_t n_windows,
                     const int32_t* pose_ptr /* n_windows + 1 */, const int32_t* pose_idx,
                     const int32_t* edge_ptr /* n_windows + 1 */, const int32_t* edge_idx,
                     const int32_t* anchor   /* n_windows */,
                     int32_t max_iters, int32_t commit,
                     double* poses_out /* pose_ptr[n_windows] x 3, or NULL */,
                     pgo_window_result* results /* n_windows */,
                     pgo_iter_record* records_or_null /* n_windows x (max_iters + 1) */);                           /* [gpu] */
int pgo_batch_window_solve(pgo_batch_t* b, int32_t n_windows, const int32_t* problem /* n_windows */,
                           const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr, const int32_t* edge_idx,
                           const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                           pgo_window_result* results, pgo_iter_record* records_or_null);                           /* [gpu] */

/* ---------------------------------------------------------------- scoring
 * How good is a result?  Ground truth of the synthetic world, the trajectory error of an estimate against a reference (ATE and
 * RPE, Sturm et al., "A Benchmark for the Evaluation of RGB-D SLAM Systems", IROS 2012), and what the robust machinery of
 * METHOD 0 / 1 did to every edge.
 *
 * pgo_synth_manhattan_truth: the ground-truth poses of the graph pgo_synth_manhattan(n_poses, *, *, seed) builds, in the frame
 * of pose 0: x = gx[i] - gx[0], y = gy[i] - gy[0], theta = wrap_pi(gh[i] pi/2) (gh[0] = 0).  The walk is the first consumer of the
 * generator's PRNG: neither edges_per_pose nor outlier_frac influences it.  The truth is comparable with the dead-reckoned initial
 * poses, which start at (0, 0, 0), and with any solve that keeps pose 0 constant, without alignment.
 * PGO_ERR_INVALID_ARG: n_poses < 2, a null pointer.                                                                          */
int pgo_synth_manhattan_truth(int32_t n_poses, uint64_t seed, double* out_xyt /* N x 3 */);     /* [host] */

/* Trajectory error of an estimate P_i = (p_i, theta_i) against a reference Q_i = (q_i, psi_i), over the COUNTED poses: those with
 * a non-zero mask byte (caller's numbering), all of them when the mask is NULL.
 * - ATE.  e_i = R(phi) p_i + t - q_i; ate_rmse = sqrt(mean |e_i|^2), ate_mean = mean |e_i|, ate_max = max |e_i| at pose
 *   ate_max_pose; rot_rmse / rot_max over |wrap(theta_i + phi - psi_i)|, wrap(a) = atan2(sin a, cos a).
 * - Alignment.  align = 0: phi = 0, t = 0.  align = 1: the rigid least-squares fit of the estimate onto the reference (Horn,
 *   no scale): centroids pbar, qbar over the counted poses; a = sum (p_i - pbar).(q_i - qbar), b = sum (p_i - pbar) x (q_i - qbar)
 *   with the 2-D cross product px qy - py qx; phi = atan2(b, a), 0 when a = b = 0; t = qbar - R(phi) pbar.  The centred sums run in
 *   a second pass after the centroids (coordinates reach +-250 m at a million poses).  (align_x, align_y, align_phi) = (t, phi).
 * - RPE over the pairs (i, i + rpe_delta) whose two ends are counted: E_i = (Q_i^-1 Q_{i+d})^-1 (P_i^-1 P_{i+d}) in SE(2),
 *   trans = |trans(E_i)|, rot = |angle(E_i)| wrapped as above; rpe_trans_rmse, rpe_trans_max (at pair rpe_max_pose = i),
 *   rpe_rot_rmse, rpe_rot_max.  RPE is invariant to the alignment and is computed on the unaligned poses.  rpe_delta = 0: none.
 * - Ties of a maximum go to the smallest index.  Nothing counted (no pose / no pair): every double of that group is 0, its index
 *   -1, and the call returns PGO_OK.
 * - per_pose (or NULL): n x 2 = (|e_i|, |wrap(theta_i + phi - psi_i)|), 0 for a pose that is not counted.
 * - A counted pose that is not finite in either trajectory: PGO_ERR_NUMERIC, pgo_last_error names the smallest such pose, the
 *   outputs are not defined.  A pose that is not counted may hold anything.
 * - PGO_ERR_INVALID_ARG: a null pointer, n < 1, align outside {0, 1}, rpe_delta < 0.
 * pgo_trajectory_error_eval is the serial evaluation on the host, in the caller's order.  pgo_trajectory_error scores the
 * handle's CURRENT poses on the device (csrc/traj_error.h is the one statement of the formulas both run): workgroups of 256
 * lanes over chunks of PGO_SCORE_POSES_PER_WG poses of the caller's numbering, per-chunk partials folded by one workgroup in
 * fixed order, no atomics; at most three passes (centroids, centred moments, errors; the last alone for align = 0); one copy-out.
 * Two calls are bitwise equal, a handle with pose_ordering 1 gives bitwise what one with 0 gives at the same poses, and the
 * result does not depend on the grid.  It agrees with pgo_trajectory_error_eval up to the association of the sums.  The handle is
 * left exactly as it was: a following pgo_lm_step gives bitwise the records and poses it gives without the call (the reference
 * and the mask go through a staging buffer of the handle's own, grown on demand: repeated calls of one size allocate nothing).
 * PGO_ERR_UNSUPPORTED: a communicator or PGO_FORCE_COLLECTIVES=1, a batched handle.  Nothing changes on error.              */
#define PGO_SCORE_POSES_PER_WG 512
typedef struct pgo_traj_options {
  int32_t align;      /* 0 (default): compare as given; 1: rigid SE(2) least-squares alignment of the estimate onto the reference */
  int32_t rpe_delta;  /* 1 (default): relative pose error over pairs (i, i + rpe_delta); 0 = none */
} pgo_traj_options;
typedef struct pgo_traj_error {
  int32_t n_poses, n_pairs;            /* counted poses / pairs */
  int32_t ate_max_pose, rpe_max_pose;  /* caller's numbering; -1 when nothing was counted; ties: the smallest index */
  double  align_x, align_y, align_phi; /* the transform applied to the estimate (0, 0, 0 for align = 0) */
  double  ate_rmse, ate_mean, ate_max; /* translation error, metres */
  double  rot_rmse, rot_max;           /* |wrap(theta_est + phi - theta_ref)| */
  double  rpe_trans_rmse, rpe_trans_max, rpe_rot_rmse, rpe_rot_max;
} pgo_traj_error;
void pgo_traj_options_default(pgo_traj_options*);                                              /* [host] */
int  pgo_trajectory_error_eval(int32_t n, const double* est_xyt, const double* ref_xyt,
                               const uint8_t* pose_mask_or_null, const pgo_traj_options* opt_or_null,
                               pgo_traj_error* out, double* per_pose_or_null /* n x 2: trans, |rot| */); /* [host] */
int  pgo_trajectory_error(pgo_t* h, const double* ref_xyt /* N x 3, caller's numbering */,
                          const uint8_t* pose_mask_or_null, const pgo_traj_options* opt_or_null,
                          pgo_traj_error* out, double* per_pose_or_null);                      /* [gpu] */

/* What the robust machinery did to each edge, METHOD 0 and 1, at the handle's current poses or at poses_or_null: one record per
 * edge in the caller's edge order.  With e the plain residual (ex, ey, asin(sin delta)) as K1 states it:
 *   s_plain = |e|^2;  scale = psi = min(1, sqrt(2 phi / (phi + ex^2 + ey^2))) on the edges METHOD 1 applies DCS to (closure and
 *   bogus), else exactly 1;  s = |scale e|^2;  rho1 = rho'(s) and cost = 1/2 rho(s) of the edge's loss class (pgo_set_losses;
 *   Huber(huber_delta) by default);  weight = scale^2 rho1 -- what the plain squared residual counts for: weight * s_plain is
 *   |r|^2 of pgo_eval's r with apply_loss != 0.  The sum of cost over the active edges is pgo_eval's cost.
 * Inactive edges (pgo_set_active) are computed too, as pgo_edge_chi2 ignores the mask; `active` says which edges count.  A
 * residual that is not finite gives NaN in every double of that record; it is not a call failure.  One lane per edge, no
 * reduction: two calls are bitwise equal.  The handle is left exactly as it was.
 * PGO_ERR_UNSUPPORTED: METHOD 2 (pgo_get_switches is its readout), info_weighting = 1 (the chi2 form of DCS is stated inside K1
 * only), a communicator or PGO_FORCE_COLLECTIVES=1, a batched handle.  PGO_ERR_INVALID_ARG: a null pointer.                  */
typedef struct pgo_edge_weight {
  double  s_plain;  /* |e|^2 of the plain residual (ex, ey, asin(sin delta)), K1's statement */
  double  scale;    /* DCS factor psi on the edges METHOD 1 applies it to, else 1 */
  double  rho1;     /* rho'(s) of the block's loss class at s = scale^2 s_plain */
  double  weight;   /* scale^2 rho1: what the plain squared residual counts for */
  double  cost;     /* 1/2 rho(s) */
  int32_t active, _pad;   /* the pgo_set_active mask */
} pgo_edge_weight;
int pgo_edge_weights(pgo_t* h, const double* poses_or_null, pgo_edge_weight* out /* E, caller's edge order */);   /* [gpu] */

/* ---------------------------------------------------------------- edge weight plane
 * A scalar weight w in [0, 1] per edge on a live handle, between the binary mask of pgo_set_active and the loss classes: with
 * a plane set, an edge counts w 1/2 rho(s) in the cost, and its residual and Jacobian rows are scaled by sqrt(w rho'(s)), s
 * being what K1 computes today (after DCS).  The plane is part of the problem like the mask: pgo_eval applies it with and
 * without apply_loss.  w = 0 gives exactly-zero rows and zero cost (as Tukey beyond its bound); the edge stays a residual
 * block, so a zero-weight odometry edge does not cut the direct solve's chain -- the rows are zero and a direct solve that
 * fails on them is redone by PCG (pgo_handle_info.direct_fallbacks).  Inactive edges stay exactly as pgo_set_active left them.
 * - A handle with a plane runs K1's general instantiation (as one with an edge mask does); the default instantiations do not
 *   read the plane.  pgo_set_edge_weights(h, NULL) restores the handle: a pgo_solve after it gives bitwise what a fresh
 *   handle gives.
 * - A solve begun with pgo_lm_begin becomes stale, as after pgo_set_losses.  pgo_set_losses and pgo_set_active leave the
 *   weights alone, in either call order.
 * - pgo_pose_covariance, pgo_edge_gate and pgo_edge_gate_joint consume K1's records: they see the WEIGHTED problem.
 *   pgo_edge_weights (scoring) reports weight = w scale^2 rho1 and cost = w 1/2 rho(s): weight * s_plain stays |r|^2 of
 *   pgo_eval's r, and the sum of cost over the active edges stays pgo_eval's cost.
 * - pgo_window_solve returns PGO_ERR_UNSUPPORTED while a plane is set (its kernel evaluates the edges itself).
 * - pgo_get_edge_weights: the plane in the caller's edge order; all ones when none is set.
 * Errors: PGO_ERR_INVALID_ARG for a weight that is not finite or outside [0, 1] (pgo_last_error names the first such edge) or a
 * null handle / output; PGO_ERR_UNSUPPORTED for METHOD 2, info_weighting = 1, a communicator or PGO_FORCE_COLLECTIVES=1, a
 * batched handle.  Nothing changes on error.                                                                                  */
int pgo_set_edge_weights(pgo_t* h, const double* w_or_null /* E, caller's edge order */);   /* [gpu] */
int pgo_get_edge_weights(pgo_t* h, double* w_out /* E */);                                  /* [gpu] */

/* ---------------------------------------------------------------- graduated non-convexity
 * GNC with the truncated-least-squares surrogate (Yang, Antonante, Tzoumas, Carlone, RA-L 2020) on the weight plane: start from
 * the convex all-edges-in problem and tighten a per-edge weight round by round.  csrc/gnc.h is the one statement:
 *   gnc_mu0(c2, rmax2) = c2 / (2 rmax2 - c2)                       (valid for 2 rmax2 > c2)
 *   gnc_tls_weight(c2, mu, s) = 1 for s <= mu / (mu + 1) c2;  0 for s >= (mu + 1) / mu c2;  else sqrt(c2 mu (mu + 1) / s) - mu
 * with c2 = cbar^2 and s = the s_plain of pgo_edge_weights: the plain |e|^2 as K1 states it, before DCS or any loss.  A
 * non-finite s gives weight 0.  pgo_gnc_weight_eval evaluates n weights on the host (cbar finite and > 0, mu finite and > 0,
 * else PGO_ERR_INVALID_ARG).
 *
 * pgo_gnc_update, at the handle's current poses: every SELECTED edge -- the active edges (pgo_set_active) with kind !=
 * PGO_EDGE_ODOMETRY, or the active edges with a non-zero byte in select (E bytes, caller's order) -- gets the weight
 * gnc_tls_weight(cbar^2, mu, s) in the handle's plane, which is allocated at all ones at its first use; every other edge keeps
 * its weight.  mu <= 0 measures only: no weight is touched (and no plane is created).  out (may be NULL) receives, over the
 * selected edges and with the weights the call leaves: n_selected; s_max, the largest finite s (-1: none); weighted_sum = sum w s
 * over the finite s; n_nonbinary, the edges with 0 < w < 1; n_zero, those with w = 0; n_nonfinite, those whose s is not finite.
 * One lane per edge of the caller's numbering, per-workgroup partials folded by one workgroup in fixed order, no atomics: two
 * calls are bitwise equal, and neither the launch grid nor the internal pose ordering plays a part.  With mu > 0 a solve begun
 * with pgo_lm_begin becomes stale.
 *
 * pgo_gnc_solve, METHOD 0, from the handle's current poses, under the handle's own options and loss:
 *   1. every selected weight <- 1; rmax2 = s_max there.
 *   2. 2 rmax2 <= cbar^2: one solve of final_iters LM iterations, rounds = 0, done.
 *   3. mu = gnc_mu0(cbar^2, rmax2).
 *   4. a round: pgo_lm_begin and up to inner_iters LM iterations; pgo_gnc_update at the new poses with mu; the round's record
 *      {mu, weighted_cost = 1/2 weighted_sum, n_nonbinary, n_zero, lm_iterations, lm_termination}; stop when n_nonbinary == 0 and
 *      this is not the first round, else mu *= mu_factor.
 *   5. after the stop, or after max_rounds rounds (hit_max_rounds = 1), one solve of final_iters with the weights as they stand.
 * (An LM solve also ends at the handle's own max_iters, whichever is smaller.)  The weights stay on the handle: for
 * pgo_get_edge_weights, for the covariances and the gates, for further solves; pgo_set_edge_weights(h, NULL) drops them.  An
 * inner solve that ends with PGO_TERM_FAILURE ends the call with PGO_ERR_NUMERIC; the poses are those of the last good round.
 * rounds_or_null receives the first rounds_cap records.
 * Errors: PGO_ERR_INVALID_ARG for a cbar that is not finite and > 0, mu_factor not finite or <= 1, inner_iters / final_iters /
 * max_rounds < 1, a NaN mu, a null handle, and for pgo_gnc_solve a handle that is not METHOD 0; PGO_ERR_UNSUPPORTED as
 * pgo_set_edge_weights.  Nothing changes on those errors.                                                                     */
typedef struct pgo_gnc_stats {
  double  s_max;          /* largest finite s over the selected edges; -1 when there is none */
  double  weighted_sum;   /* sum of w s over the selected edges with a finite s */
  int32_t n_selected, n_nonbinary, n_zero, n_nonfinite;
} pgo_gnc_stats;
typedef struct pgo_gnc_options {
  double  cbar;           /* no default: finite and > 0 -- the residual norm above which an edge is an outlier */
  double  mu_factor;      /* 1.4 */
  int32_t inner_iters;    /* 5 */
  int32_t final_iters;    /* 50 */
  int32_t max_rounds;     /* 100 */
  int32_t _pad;
  const uint8_t* select;  /* NULL: the active edges with kind != PGO_EDGE_ODOMETRY; else E bytes, caller's order */
} pgo_gnc_options;
typedef struct pgo_gnc_round {
  double  mu, weighted_cost;
  int32_t n_nonbinary, n_zero, lm_iterations, lm_termination;
  double  seconds;        /* the round's wall time: inner solve + update */
} pgo_gnc_round;
typedef struct pgo_gnc_summary {
  int32_t rounds, hit_max_rounds;
  int32_t n_selected, n_zero;       /* selected edges; those at weight 0 when the call returns */
  double  rmax2, mu0, mu_last;      /* mu0 = mu_last = 0 when rounds == 0 */
  double  seconds_total;
  pgo_summary final_solve;          /* the solve of step 2 / 5 */
} pgo_gnc_summary;
void pgo_gnc_options_default(pgo_gnc_options*);   /* cbar = 0: the caller must set it */                          /* [host] */
int  pgo_gnc_weight_eval(double cbar, double mu, int32_t n, const double* s, double* w_out);                      /* [host] */
int  pgo_gnc_update(pgo_t* h, double cbar, double mu, const uint8_t* select_or_null, pgo_gnc_stats* out_or_null); /* [gpu] */
int  pgo_gnc_solve(pgo_t* h, const pgo_gnc_options* opt, pgo_gnc_summary* summary_or_null,
                   pgo_gnc_round* rounds_or_null, int32_t rounds_cap);                                            /* [gpu] */

/* ---------------------------------------------------------------- max-mixture edges
 * Max-Mixtures (Olson & Agarwal, RSS 2012 / IJRR 2013): an edge that is ONE OF SEVERAL measurements -- a loop closure that
 * matches either of two corridors, an odometry step that happened or slipped, an inlier beside a wide null hypothesis.  Per
 * edge and per linearisation point the most likely component is selected, and an ordinary Gaussian problem is optimised.  On a
 * live handle the component of an edge is its entries of the measurement planes and of the edge weight plane; csrc/mixture.h is
 * the one statement:
 * - A mixture edge is an edge of the handle (caller's edge numbering) with K components, 1 <= K <= PGO_MIX_MAX_COMPONENTS.
 *   Component k has a mean meas = (x, y, theta), a mixing weight weight = pi_k > 0 (relative: the weights need not sum to 1)
 *   and an information scale info_scale = w_k in (0, 1]: in the handle's unit-information objective its information is w_k I.
 *   Its constant is c_k = -log(pi_k) - 1.5 log(w_k), computed once on the host in double.
 * - At poses x, s_k(x) is the plain |e|^2 for the measurement m_k -- the s_plain of pgo_edge_weights, heading asin(sin delta) --
 *   and q_k(x) = w_k 1/2 rho(s_k) + c_k with rho the loss of the edge's loss class (pgo_set_losses).  A component whose s_k is
 *   not finite has no q_k (NaN), whatever the loss.
 * - Selection: k* = argmin q_k over the components with a finite q_k, ties to the lowest index.  Without a finite component
 *   the edge keeps the selection it has and is counted in n_nonfinite.
 * - Applying a selection writes m_k* into the edge's measurement planes and w_k* into its entry of the edge weight plane, which
 *   is allocated at all ones at its first use (as pgo_gnc_update).
 * Because q_k is stated with the handle's own loss and weight, F(x) = pgo_eval's cost under the applied selection + the sum of
 * c_k* over the (active) mixture edges is non-increasing from round to round of pgo_mixture_solve, for any loss: with the
 * selection fixed LM never raises its cost, and re-selecting at the new poses never raises any edge's q.
 *
 * pgo_set_mixtures stores the table: edge[n_mix] strictly ascending, comp_ptr[n_mix + 1] the CSR offsets into comps
 * (comp_ptr[0] = 0).  No selection is applied yet and no plane is touched.  n_mix = 0 clears: the measurement planes of the
 * former mixture edges are restored bitwise to what the handle was created with, their weights (if a plane is set) become 1,
 * the table is dropped; after it and pgo_set_edge_weights(h, NULL), pgo_solve gives bitwise what a fresh handle gives.  Setting
 * a new table over an old one clears the old one first.
 * pgo_set_mixture_null is the classic robust use without a host table: every selected edge -- the active edges with kind !=
 * PGO_EDGE_ODOMETRY, or the active edges with a non-zero byte in select (E bytes) -- gets two components at the mean it was
 * created with, (pi = 1, w = 1) and (pi_null, scale_null): exactly the table pgo_set_mixtures would be given, in ascending
 * edge order.  No selected edge, or a (pi_null, scale_null) that no component may have: PGO_ERR_INVALID_ARG.
 *
 * pgo_mixture_select runs the selection at the handle's current poses.  apply = 0 measures only: nothing is written and no
 * plane is created.  chosen_or_null[n_mix] receives the component per mixture edge (an edge that was not evaluated: the
 * selection it has, -1 where none); q_or_null[2 n_mix] receives q_best and the margin q_second - q_best (+inf with one finite
 * component; NaN for both on an edge that was not evaluated).  stats: n_mix; n_changed, against the previous APPLIED selection
 * (the first apply counts every evaluated edge); n_nonfinite; n_inactive -- edges masked by pgo_set_active keep their selection
 * and their planes and count only here; offset = the sum of c_k* and mix_cost = the sum of q_k* over the evaluated edges;
 * count[k] = the evaluated edges on component k.  One lane per mixture edge, per-chunk partials folded by one workgroup in
 * fixed order, no atomics: two calls are bitwise equal, and neither the launch grid ("mix_grid") nor pose_ordering plays a
 * part.  An applying select makes a solve begun with pgo_lm_begin stale, as pgo_gnc_update does (it rewrites the weights of
 * its edges whether or not the selection moved: another writer may have been there).
 * pgo_get_mixture_selection: the last applied selection per mixture edge, -1 where none.
 *
 * pgo_mixture_solve, METHOD 0, from the handle's current poses, under the handle's own options and losses.  A round:
 *   1. select + apply;  2. the round's record {objective F, n_changed, count[], lm_iterations, lm_termination, seconds} (the LM
 *   figures are those of step 4);  3. stop if this is not the first round and n_changed == 0;  4. pgo_lm_begin and up to
 *   inner_iters LM iterations.
 * After the stop, or after max_rounds rounds (hit_max_rounds = 1), one solve of final_iters, then one measuring select whose
 * n_changed goes to n_would_change.  (An LM solve also ends at the handle's own max_iters, whichever is smaller.)  An inner
 * solve that ends with PGO_TERM_FAILURE ends the call with PGO_ERR_NUMERIC; the poses are those of the last good round.
 *
 * Host only: pgo_mixture_eval is the statement on given s[n_comp] under one loss (NULL: Trivial); chosen = -1 and NaN when no
 * component is finite.  pgo_mixture_plan is the whole select on arrays, serially, the sums in the caller's mixture order:
 * mix_class[n_mix] is each mixture edge's loss class (NULL: class 0; losses NULL: Trivial), prev_or_null the previous applied
 * selection (NULL: none, -1), active_or_null a byte per mixture edge (NULL: all active).
 *
 * Interplay: pgo_set_edge_weights and pgo_gnc_update may overwrite a mixture edge's weight and the next applied select
 * overwrites it again -- last writer wins.  pgo_set_losses and pgo_set_active leave the table and the selection alone.
 * pgo_window_solve stays PGO_ERR_UNSUPPORTED while a plane is set.  Everything that reads the planes -- pgo_eval and the solves,
 * pgo_edge_weights, the covariances and the gates, pgo_coarsen, pgo_loop_support, pgo_chordal_init -- sees the selected problem
 * (an apply that changes a measurement drops the trajectory pgo_loop_support keeps and the composites pgo_prolong relies on).
 * Errors: PGO_ERR_INVALID_ARG for a null pointer, an edge list that is not strictly ascending or out of range, K outside 1 ..
 * 8, a mean that is not finite, a weight that is not finite or <= 0, an info_scale that is not finite or outside (0, 1]
 * (pgo_last_error names the first offending edge), pgo_mixture_select / pgo_mixture_solve / pgo_get_mixture_selection without
 * a table, inner_iters / final_iters / max_rounds < 1; PGO_ERR_UNSUPPORTED for METHOD 1 or 2, info_weighting = 1, a
 * communicator or PGO_FORCE_COLLECTIVES=1, a batched handle.  Nothing changes on error.                                        */
#define PGO_MIX_MAX_COMPONENTS 8
typedef struct pgo_mix_component {
  double meas[3];      /* the mean (x, y, theta) */
  double weight;       /* pi_k > 0, relative */
  double info_scale;   /* w_k in (0, 1] */
} pgo_mix_component;
typedef struct pgo_mix_stats {
  int32_t n_mix, n_changed, n_nonfinite, n_inactive;
  double  offset;      /* sum of c_k* over the evaluated edges */
  double  mix_cost;    /* sum of q_k* over the evaluated edges */
  int32_t count[PGO_MIX_MAX_COMPONENTS];
} pgo_mix_stats;
typedef struct pgo_mixture_options {
  int32_t inner_iters;    /* 2 */
  int32_t final_iters;    /* 50 */
  int32_t max_rounds;     /* 50 */
  int32_t _pad;
} pgo_mixture_options;
typedef struct pgo_mixture_round {
  double  objective;      /* F = pgo_eval's cost under the round's selection + offset */
  int32_t n_changed, lm_iterations, lm_termination, _pad;
  int32_t count[PGO_MIX_MAX_COMPONENTS];
  double  seconds;        /* the round's wall time: select + inner solve */
} pgo_mixture_round;
typedef struct pgo_mixture_summary {
  int32_t rounds, hit_max_rounds;
  int32_t n_mix, n_would_change;    /* n_changed of a measuring select at the final poses */
  double  objective, offset;        /* F and the sum of c_k* at the final poses, under the selection in force */
  double  seconds_total;
  pgo_summary final_solve;
} pgo_mixture_summary;
void pgo_mixture_options_default(pgo_mixture_options*);                                                           /* [host] */
int  pgo_mixture_eval(int32_t n_comp, const pgo_mix_component* comps, const double* s, const pgo_loss* loss_or_null,
                      int32_t* chosen, double* q_best, double* margin);                                           /* [host] */
int  pgo_mixture_plan(int32_t n_poses, const double* poses, int32_t n_edges, const int32_t* ia, const int32_t* ib,
                      int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps,
                      int32_t n_classes, const pgo_loss* losses_or_null, const uint8_t* mix_class_or_null,
                      const int32_t* prev_or_null, const uint8_t* active_or_null,
                      int32_t* chosen /* n_mix */, double* q /* 2 n_mix */, pgo_mix_stats* stats_or_null);         /* [host] */
int  pgo_set_mixtures(pgo_t* h, int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps); /* [gpu] */
int  pgo_set_mixture_null(pgo_t* h, const uint8_t* select_or_null, double pi_null, double scale_null);            /* [gpu] */
int  pgo_mixture_select(pgo_t* h, int32_t apply, pgo_mix_stats* stats_or_null, int32_t* chosen_or_null, double* q_or_null); /* [gpu] */
int  pgo_get_mixture_selection(pgo_t* h, int32_t* chosen_out /* n_mix */);                                        /* [gpu] */
int  pgo_mixture_solve(pgo_t* h, const pgo_mixture_options* opt_or_null, pgo_mixture_summary* summary_or_null,
                       pgo_mixture_round* rounds_or_null, int32_t rounds_cap);                                    /* [gpu] */

/* ---------------------------------------------------------------- loop support (odometry cycle consistency)
 * Judge loop edges WITHOUT looking at the estimate: two loop closures taken a few steps apart must close a 4-cycle through the
 * odometry between their ends (the pairwise check of PCM / RRR, restricted to neighbours along the chain, where the odometry
 * path is short and the test is sharp).  Caller's numbering throughout; csrc/loop_support.h is the one statement.
 * - Chain.  As pgo_coarsen: the pair (i, i + 1) is joined by the first edge between the two in the caller's order, in either
 *   orientation; Z_i is its motion from i to i + 1.  A pair without one: PGO_ERR_UNSUPPORTED, pgo_last_error names the first.
 * - Trajectory.  T_0 = (0, 0, 0), T_{i+1} = T_i o Z_i (angles plain sums, not wrapped); O(p, q) = T_p^-1 o T_q.
 * - Selected loops.  An edge that is not a chain edge and either select == NULL and kind != PGO_EDGE_ODOMETRY, or its byte in
 *   select (E bytes, caller's order) is non-zero.  A chain edge named by select is simply not selected.  The pgo_set_active mask
 *   plays no part (as in pgo_edge_chi2 and pgo_coarsen): this is the test that decides what to activate.
 * - Canonical form of the loop e = (a, b, m): lo = min(a, b), hi = max(a, b), M_e = m if a < b, else m^-1.
 * - Neighbours.  f is a neighbour of e when f is selected, f != e as an edge index (duplicates of e count),
 *   |lo_e - lo_f| <= window and |hi_e - hi_f| <= window.
 * - Cycle error of the pair: Err = M_e o O(hi_e, hi_f) o M_f^-1 o O(lo_f, lo_e).  With L = |lo_e - lo_f| + |hi_e - hi_f|,
 *     q(e, f) = max((Err.x^2 + Err.y^2) / (tol_xy^2 (2 + L)), wrap(Err.th)^2 / (tol_th^2 (2 + L)));
 *   the pair is consistent iff q <= 1; a q that is not finite is not consistent.
 * - Every edge gets one `struct pgo_loop_support` record, in the caller's order; an edge that is not selected gets
 *   {selected 0, n_pairs 0, n_consistent 0, best -1, q_min -1}.  The totals run over the selected edges.
 * - Errors.  A selected or chain measurement that is not finite: PGO_ERR_NUMERIC, pgo_last_error names the smallest such edge.
 *   PGO_ERR_INVALID_ARG: window outside 1 .. PGO_LOOP_SUPPORT_MAX_WINDOW, tol_xy or tol_th not finite or not > 0,
 *   min_support < 1, a null pointer, n_poses < 2, an endpoint out of range.
 * - Defaults: window 32, tol_xy 0.1, tol_th 0.05, min_support 1, apply 0.  The tolerances are five times the per-step odometry
 *   noise of pgo_synth_manhattan (0.02 m, 0.01 rad): they are the allowance per sqrt(step) of odometry in the cycle.  A REAL
 *   DATASET NEEDS THE CALLER'S OWN VALUES, from its odometry's noise.
 * pgo_loop_support_plan is the serial statement on arrays: T folded left to right (T_or_null receives it, N x 3); the
 * neighbours may be scanned in any order -- the counts and the minimum (ties to the smallest edge index) do not depend on it.
 * pgo_loop_support runs the same statement on the measurements the handle holds on the device.  T is a three-level scan (one
 * wavefront per segment of 256 poses folds and scans its chain motions, one workgroup scans the segment ends, one lane per
 * pose composes the two), the selected loops are sorted by (lo, edge index) on the host at the first call for a selection and
 * kept with a first[] array over the poses, so that a loop's candidates are one contiguous range of the table, and
 * k_loop_support takes one loop per lane in that order.  No atomics, fixed trees: two calls are bitwise equal, a handle with
 * pose_ordering 1 gives bitwise what one with 0 gives, and the grid plays no part; the result agrees with the plan up to the
 * association of the compositions in T.
 * With opt.apply != 0 every selected edge gets the weight 1 if n_consistent >= min_support, else 0, in the handle's edge weight
 * plane (created at all ones at its first use; every other edge keeps its weight -- as pgo_gnc_update); a solve begun with
 * pgo_lm_begin is stale afterwards, and the refusals are those of pgo_set_edge_weights.  With apply == 0 any METHOD and
 * info_weighting are fine, no plane is created and the handle is left exactly as it was: a following pgo_lm_step gives
 * bitwise the records and poses it gives without the call.
 * PGO_ERR_UNSUPPORTED: a communicator, PGO_FORCE_COLLECTIVES=1, a batched handle.  Nothing changes on error.                 */
#define PGO_LOOP_SUPPORT_MAX_WINDOW 256
typedef struct pgo_loop_support_options {
  int32_t window;         /* 32 */
  int32_t min_support;    /* 1 */
  int32_t apply;          /* 0 */
  int32_t _pad;
  double  tol_xy;         /* 0.1 */
  double  tol_th;         /* 0.05 */
} pgo_loop_support_options;
struct pgo_loop_support {   /* (a tag only: the name is also the [gpu] call's; pgo_loop_support_record is its typedef) */
  int32_t selected;       /* 0 or 1 */
  int32_t n_pairs;        /* number of neighbours */
  int32_t n_consistent;   /* number of consistent neighbours */
  int32_t best;           /* edge index of the neighbour with the smallest finite q (ties: the smallest index); -1 if none */
  double  q_min;          /* that q; -1 if none */
};
typedef struct pgo_loop_support pgo_loop_support_record;
typedef struct pgo_loop_support_stats {
  int64_t n_pairs_total;
  int32_t n_selected;
  int32_t n_supported;    /* selected edges with n_consistent >= min_support */
  int32_t max_pairs;
  int32_t _pad;
} pgo_loop_support_stats;
void pgo_loop_support_options_default(pgo_loop_support_options*);                                                 /* [host] */
int  pgo_loop_support_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas_xyt,
                           const uint8_t* kind, const uint8_t* select_or_null, const pgo_loop_support_options* opt,
                           pgo_loop_support_record* out /* E */, pgo_loop_support_stats* stats, double* T_or_null /* N x 3 */); /* [host] */
int  pgo_loop_support(pgo_t* h, const pgo_loop_support_options* opt, const uint8_t* select_or_null,
                      pgo_loop_support_record* out_or_null /* E */, pgo_loop_support_stats* stats_or_null);               /* [gpu] */

/* ---------------------------------------------------------------- hierarchical initialisation
 * Start a large solve near its answer (HOG-Man style): collapse every `stride` consecutive poses onto a key pose, carry every
 * other edge to the key poses along the odometry chain, solve that small graph exactly with a handle of its own, and spread the
 * result back over the fine poses.  Caller's numbering throughout; csrc/coarsen.h is the one statement of the operators.
 * - Sizes.  PGO_COARSEN_MIN_STRIDE <= S <= PGO_COARSEN_MAX_STRIDE; key pose k is fine pose kS, K = ceil(N / S) of them;
 *   N <= S is PGO_ERR_INVALID_ARG.
 * - Chain.  The pair (i, i + 1) is joined by its chain edge: the first edge between the two in the caller's order, in either
 *   orientation -- the odometry chain of the direct solve.  Z_i is its measurement as a motion from i to i + 1 (inverted for an
 *   edge stored as (i + 1, i)).  A pair without one: PGO_ERR_UNSUPPORTED, pgo_last_error names the first.
 * - Composites.  C_i = Z_{kS} o ... o Z_{i-1} for kS < i < (k+1)S, C_{kS} = (0, 0, 0) exactly; Cend_k = C_{(k+1)S-1} o Z_{(k+1)S-1}
 *   for k < K - 1.  Their angles are plain sums, not wrapped.
 * - Coarse edges, in this order: the K - 1 composites (k, k + 1, Cend_k), kind PGO_EDGE_ODOMETRY, origin -1; then every fine
 *   edge e = (a, b, m) that is not a chain edge and has a / S != b / S, in the caller's edge order, as
 *   (a / S, b / S, C_a o m o C_b^-1) with orientation and kind kept and origin = e.  Theta of every coarse measurement is wrapped
 *   with atan2(sin, cos).  Edges inside one segment are dropped; parallel coarse edges are not merged.
 * - The coarse graph of pgo_coarsen / pgo_coarsen_plan carries NO information matrices (unit information); "with information"
 *   below propagates them.  The pgo_set_active mask is ignored, as pgo_edge_chi2 ignores it; origin lets the caller mask the coarse graph.
 * - A measurement that is not finite: PGO_ERR_NUMERIC, pgo_last_error names the smallest such edge.
 * - Prolongation of coarse poses X (K x 3), with t = (i - kS) / S: F_i = X_k o C_i; for k < K - 1, B_i = X_{k+1} o Cend_k^-1 o C_i
 *   and P_i = ((1-t) F_x + t B_x, (1-t) F_y + t B_y, F_th + t wrap(B_th - F_th)); the last segment is forward only, P_i = F_i.
 *   Key poses come back bitwise: P_{kS} = X_k.
 * pgo_coarsen_plan is the serial statement on arrays (composites folded left to right): it fills n_coarse_poses, the coarse
 * lists and, optionally, C (N x 3) and Cend ((K - 1) x 3).  A cap that is too small: the counts are still returned, the lists
 * are not written, PGO_ERR_INVALID_ARG.  pgo_prolong_eval is the serial prolongation.
 * pgo_coarsen does the same on a live handle, from the measurements it holds on the device, and returns a graph ready for
 * pgo_create_from_graph (free it with pgo_graph_free) whose initial poses are the handle's CURRENT poses at the key poses;
 * origin_or_null (origin_cap entries) receives the origin of every coarse edge, n_coarse_edges_or_null their number (also when
 * the cap is too small: PGO_ERR_INVALID_ARG then).  One wavefront per segment scans the chain motions under SE(2)
 * composition (up to 4 consecutive poses per lane folded serially, then a log-step scan over the lanes; the rotation is
 * carried as (cos, sin), one sincos per motion); one lane per fine edge transports it, kept edges are compacted stably
 * (per-chunk counts, one workgroup scans them, a second pass writes each edge to its slot); one copy-out.  No floating-point
 * atomics: two calls are bitwise equal, a handle with pose_ordering 1 gives bitwise what one with 0 gives, and the grid plays
 * no part; the result agrees with pgo_coarsen_plan up to the association of the compositions.  C and Cend of that stride stay
 * on the device, in buffers of the handle's own, grown on demand and kept.  The handle is otherwise left exactly as it was: a
 * following pgo_lm_step gives bitwise the records and poses it gives without the call.
 * pgo_prolong writes the prolongation of coarse_xyt into the handle's poses on the device, as pgo_set_poses would (a solve
 * begun with pgo_lm_begin is stale afterwards).  The resolved constant poses (opt.fixed_pose, and under pgo_set_active the
 * poses it resolved to constant) are not moved.  Without a preceding pgo_coarsen of the same stride: PGO_ERR_INVALID_ARG.  A
 * coarse pose that is not finite: PGO_ERR_NUMERIC.
 * PGO_ERR_UNSUPPORTED ([gpu] calls): a communicator, PGO_FORCE_COLLECTIVES=1, a batched handle.  Any METHOD and info_weighting
 * are fine: these are graph operations.  Nothing changes on error.                                                            */
#define PGO_COARSEN_MIN_STRIDE 2
#define PGO_COARSEN_MAX_STRIDE 256
int pgo_coarsen_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas_xyt,
                     const uint8_t* kind, int32_t stride, int32_t* n_coarse_poses_out,
                     int32_t edge_cap, int32_t* coarse_ia, int32_t* coarse_ib, double* coarse_meas /* cap x 3 */,
                     uint8_t* coarse_kind, int32_t* coarse_origin, int32_t* n_coarse_edges_out,
                     double* C_or_null /* N x 3 */, double* Cend_or_null /* (K - 1) x 3 */);                     /* [host] */
int pgo_prolong_eval(int32_t n_poses, int32_t stride, const double* C /* N x 3 */, const double* Cend /* (K - 1) x 3 */,
                     const double* coarse_xyt /* K x 3 */, double* out_xyt /* N x 3 */);                         /* [host] */
int pgo_coarsen(pgo_t* h, int32_t stride, pgo_graph** coarse_out, int32_t* origin_or_null, int32_t origin_cap,
                int32_t* n_coarse_edges_or_null);                                                                /* [gpu] */
int pgo_prolong(pgo_t* h, int32_t stride, const double* coarse_xyt /* K x 3 */);                                 /* [gpu] */
/* With information.  pgo_coarsen_info_plan and pgo_coarsen_info are pgo_coarsen_plan and pgo_coarsen with the edges' information
 * matrices carried through the composition: same key poses, same coarse edges in the same order, same measurements.
 * - A pair (A, Sigma_A) couples a motion with the covariance of ADDITIVE noise on its own triple (x, y, theta) -- what a g2o
 *   information matrix is the inverse of.  Covariances are six doubles in the order of info6 (xx, xy, xt, yy, yt, tt).
 *     (A, Sigma_A) o (B, Sigma_B) = (A o B, F Sigma_A F' + G Sigma_B G')
 *        F = [1 0 -(s_A B.x + c_A B.y); 0 1 c_A B.x - s_A B.y; 0 0 1],  G = [c_A -s_A 0; s_A c_A 0; 0 0 1]
 *     (A, Sigma_A)^-1 = (B, H Sigma_A H'),  B = A^-1,  H = [-c_A -s_A B.y; s_A -c_A -B.x; 0 0 -1]
 *   First order in the noise; the identity pair is ((0, 0, 0), 0).  The covariance of a product does not depend on how it is
 *   associated (chain rule), so the device's trees and the plan's serial fold agree up to rounding.
 * - Z_i is the pair (m, Omega^-1) of its chain edge, inverted for an edge stored as (i + 1, i); C_i and Cend_k follow as above,
 *   as pairs.  Composite k carries the information Sigma(Cend_k)^-1.  A kept edge e = (a, b, m, Omega) carries the inverse of the
 *   covariance of pair(C_a) o (m, Omega^-1) o pair(C_b)^-1 (a and b lie in different segments: three independent factors).
 *   Omega^-1 and Sigma^-1 are formed by Cholesky factorisation (the edge gate's), inverting the factor and multiplying.
 *   Wrapping an angle does not touch a covariance.  A handle created without information matrices, or info6_or_null = NULL,
 *   uses Omega = I on every edge.
 * - Coarse edges that share chain motions -- the edges that leave or enter one segment, and that segment's composite -- are
 *   CORRELATED.  The coarse graph treats them as independent: that correlation is ignored.
 * - The coarse objective is in units of the fine information.  A robust kernel's scale on the coarse graph is the caller's to
 *   choose: with info_weighting = 1 the DCS parameter phi of METHOD 1 acts on chi2 (on synth_manhattan(2000, 4.0, 0.1, 3),
 *   stride 16, unit fine information: phi 0.5 leaves a prolonged start 10.4 m off, phi 5 gives 0.208 m).
 * - PGO_ERR_NUMERIC, pgo_last_error naming the smallest such edge: a chain edge, or a kept edge of this stride, whose information
 *   matrix is not finite and positive definite -- found before anything is written.  An edge this stride drops may hold
 *   anything.  (A g2o EDGE2 file read positionally gives indefinite matrices: an error, not a graph.)  A coarse covariance that
 *   lost positive definiteness to rounding is PGO_ERR_NUMERIC as well.
 * pgo_coarsen_info_plan: pgo_coarsen_plan's arguments, info6_or_null (E x 6) in; coarse_info and coarse_cov (edge_cap x 6, either
 * may be NULL) and, optionally, the covariances of C (N x 6) and of Cend ((K - 1) x 6) out.  Serial, folded left to right.
 * pgo_coarsen_info: pgo_coarsen's arguments and cov_or_null (cap x 6; cap counts the entries of origin_or_null and of
 * cov_or_null alike).  The graph it returns carries the propagated information.  It leaves C and Cend of that stride on the
 * handle exactly as pgo_coarsen does: pgo_prolong works after either.  Kernels of its own -- one wavefront per segment scans
 * pairs in pgo_coarsen's tree (the lane's motions are folded once for the scan and again for the write-out), one lane per kept
 * edge writes measurement, covariance and information to pgo_coarsen's slots -- and still one copy-out.  The information
 * matrices are checked on the host, once per handle: the handle keeps no host copy of them, so the FIRST pgo_coarsen_info on a
 * handle copies the six planes back (48 bytes per edge, about 190 MB at 4M edges) and factors every matrix; later calls, at
 * any stride, read one flag per edge.  Everything pgo_coarsen promises holds: no atomics, two calls bitwise
 * equal, pose_ordering and "coarsen_grid" play no part, the LM state is untouched, buffers grown on demand and kept.          */
int pgo_coarsen_info_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas_xyt,
                          const uint8_t* kind, const double* info6_or_null /* E x 6 */, int32_t stride, int32_t* n_coarse_poses_out,
                          int32_t edge_cap, int32_t* coarse_ia, int32_t* coarse_ib, double* coarse_meas /* cap x 3 */,
                          uint8_t* coarse_kind, int32_t* coarse_origin, double* coarse_info_or_null /* cap x 6 */,
                          double* coarse_cov_or_null /* cap x 6 */, int32_t* n_coarse_edges_out,
                          double* C_or_null /* N x 3 */, double* Cend_or_null /* (K - 1) x 3 */,
                          double* Ccov_or_null /* N x 6 */, double* Cendcov_or_null /* (K - 1) x 6 */);           /* [host] */
int pgo_coarsen_info(pgo_t* h, int32_t stride, pgo_graph** coarse_out, int32_t* origin_or_null, double* cov_or_null /* cap x 6 */,
                     int32_t cap, int32_t* n_coarse_edges_or_null);                                               /* [gpu] */

/* ---------------------------------------------------------------- chordal initialisation (an estimate-free linear start)
 * Poses from the measurements alone, by the two-stage linear relaxation of SE(2) (chordal rotations, then positions given the
 * rotations: Martinec-Pajdla, LAGO, Carlone's "initialization techniques"): no basin, no estimate.  Both stages are one kind of
 * system -- a Hermitian, complex-valued weighted graph Laplacian with a unit phase per edge -- solved by Jacobi-preconditioned
 * CG.  Caller's numbering throughout; csrc/chordal.h is the one statement.
 * - Weights.  Edge e = (a, b, m) has u_e = its weight (the edge weight plane, 1 without one; w of pgo_chordal_plan) if it is
 *   active (pgo_set_active), else 0.  An edge with a == b has u_e = 0.
 * - Constant poses C: what the handle holds constant (opt.fixed_pose, and under pgo_set_active the poses it resolved to
 *   constant); constant_or_null of pgo_chordal_plan (NULL: pose 0).  They keep their current values.  c0 = the smallest.
 * - Chain and trajectory: as pgo_loop_support -- the first edge between i and i + 1 in the caller's order, T_0 = (0, 0, 0),
 *   T_{i+1} = T_i o Z_i, whatever the weight of the chain edge.  X_i = (P_c0 o T_c0^-1) o T_i is T moved rigidly onto c0.
 * - Stage R.  Unknowns z_i complex, z_c = exp(i theta_c) on C: minimise sum_e u_e |z_b - exp(i m_theta) z_a|^2.  Then
 *   theta_i = atan2(Im z_i, Re z_i), zh_i = z_i / |z_i|.  A pose with |z_i| < mag_min is degenerate: it is counted and keeps the
 *   heading of X_i.
 * - Stage T.  Unknowns t_i complex, t_c = x_c + i y_c on C: minimise sum_e u_e |t_b - t_a - zh_a (m_x + i m_y)|^2.
 * - Both are H x = b with H_aa += u, H_bb += u, H_ba -= u phi, H_ab -= u conj(phi), phi = exp(i m_theta) in stage R and 1 in
 *   stage T; the rows of C are eliminated (identity rows, their coupling moved into b).  A pose that is not constant and has no
 *   positive-weight edge is an identity row as well: it keeps X_i.  Jacobi-PCG from x0 = X (stage R: its rotation) until
 *   |r| <= rtol |b|, at most max_iters iterations; |r| and |b| run over the rows that are not identity rows.
 * - Report per edge, caller's order: res_out[2e] = |t_b - t_a - zh_a m|, res_out[2e + 1] = |wrap(theta_b - theta_a - m_theta)|.
 * - Reject rounds.  After each of the first `rounds` solves every edge with u_e > 0 that is not a chain edge and has
 *   res_xy > reject_xy or res_th > reject_th gets u_e = 0, and the system is solved again; the rounds end early when a solve
 *   rejects nothing.  The last solve rejects nothing.  With apply_weights the rejected edges get the weight 0 in the handle's
 *   edge weight plane (created at all ones at its first use, every other edge keeps its weight; a solve begun with
 *   pgo_lm_begin is stale afterwards; the refusals are those of pgo_set_edge_weights).
 * - commit != 0 writes (Re t, Im t, theta) as the handle's poses, as pgo_prolong does: the constant poses stay bitwise as they
 *   were and a solve begun with pgo_lm_begin is stale.  With commit == 0 and apply_weights == 0 the handle is left exactly as it
 *   was: a following pgo_lm_step gives bitwise the records and poses it gives without the call.
 * - Errors.  PGO_ERR_UNSUPPORTED: a component of the positive-weight edges without a constant pose (pgo_last_error names one of
 *   its poses) -- at the start or after a round's rejections --, a pair (i, i + 1) without an edge, a communicator,
 *   PGO_FORCE_COLLECTIVES=1, a batched handle.  PGO_ERR_NUMERIC: a measurement of a positive-weight edge or of a chain edge
 *   that is not finite (pgo_last_error names the smallest such edge); a solution that is not finite.  PGO_ERR_INVALID_ARG: rtol
 *   not finite or <= 0, max_iters < 1, check_every < 1, mag_min < 0, rounds outside 0 .. PGO_CHORDAL_MAX_ROUNDS, a reject
 *   threshold that is NaN or <= 0, a null pointer, n_poses < 2, an endpoint out of range, a weight outside [0, 1].  Nothing
 *   changes on error.
 * pgo_chordal_plan is the serial statement on arrays (sums in the caller's order, the convergence test after every iteration).
 * pgo_chordal_init runs it on the measurements the handle holds on the device.  The slot table (rows sorted by (pose, edge
 * index), col and edge | orientation per slot, duplicates keep their slots) is built on the host once per handle; per stage
 * k_chordal_assemble writes the 16-byte slot values, the real diagonal (summed in slot order), b and x0; k_chordal_spmv gives a
 * wavefront 64 consecutive rows, whose slots are contiguous -- its lanes stride them with 16-byte value loads and gather x[col]
 * as 16 bytes, the products of a row are added in slot order -- and writes the partials of Re(p^H q) of its tile of 256 rows;
 * two fused vector kernels fold the partials in fixed order into alpha and beta and update x, r, z = r / d and p: three
 * launches per iteration.  The host reads the residual norm once per check_every iterations: the device stops by itself at
 * the iteration the plan stops at, the launches after it do nothing.  No atomics, fixed trees: two calls are bitwise equal, a
 * handle with pose_ordering 1 gives bitwise what one with 0 gives, and the grid ("chordal_grid") plays no part; the result
 * agrees with the plan up to the association of the dot products and of T.  fp64 throughout.                                  */
#define PGO_CHORDAL_MAX_ROUNDS 8
typedef struct pgo_chordal_options {
  double  rtol;           /* 1e-8 */
  double  mag_min;        /* 1e-3 */
  double  reject_xy;      /* 2.0 (metres) */
  double  reject_th;      /* 0.35 (radians) */
  int32_t max_iters;      /* 20000, per stage */
  int32_t check_every;    /* 50 */
  int32_t rounds;         /* 0 */
  int32_t commit;         /* 0 */
  int32_t apply_weights;  /* 0 */
  int32_t _pad;
} pgo_chordal_options;
typedef struct pgo_chordal_solve {   /* one solve of both stages: [0] stage R, [1] stage T */
  int32_t iters[2];
  int32_t converged[2];
  double  rel_residual[2];   /* |r| / |b| at the end (the recurrence residual) */
  double  min_mag;           /* the smallest |z_i| over the poses that are not constant (+inf: none; NaN: some |z_i| is) */
  int32_t n_degenerate;
  int32_t n_rejected;        /* edges this solve's residuals rejected */
} pgo_chordal_solve;
typedef struct pgo_chordal_summary {
  int32_t n_solves;          /* 1 + the reject rounds that ran */
  int32_t n_rejected;        /* in all */
  int32_t n_degenerate;      /* of the last solve, as min_mag */
  int32_t _pad;
  double  min_mag;
  double  seconds;
  pgo_chordal_solve solve[PGO_CHORDAL_MAX_ROUNDS + 1];
} pgo_chordal_summary;
void pgo_chordal_options_default(pgo_chordal_options*);                                                           /* [host] */
int  pgo_chordal_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas_xyt,
                      const double* w_or_null /* E */, const uint8_t* constant_or_null /* N */, const double* poses_xyt /* N x 3 */,
                      const pgo_chordal_options* opt, double* poses_out /* N x 3 */, double* res_out /* E x 2 */,
                      double* w_out_or_null /* E: w with 0 on the rejected edges */, pgo_chordal_summary* summary);   /* [host] */
int  pgo_chordal_init(pgo_t* h, const pgo_chordal_options* opt, double* poses_out_or_null /* N x 3 */,
                      double* res_out_or_null /* E x 2 */, pgo_chordal_summary* summary_or_null);                    /* [gpu] */

/* ---------------------------------------------------------------- pose priors (absolute, unary SE(2) factors)
 * "Pose i is at z, with information Lambda": a GPS or survey fix, a known start or end pose, a position-only anchor -- g2o's
 * EDGE_PRIOR_SE2, a one-block AddResidualBlock in Ceres.  Every other residual block here joins two poses; the only gauge a
 * handle had was hard (fixed_pose, pose_constant).  csrc/prior.h is the one statement:
 *   d    = (x_i - z_x, y_i - z_y, remainder(theta_i - z_theta, 2 pi))   the IEEE remainder: d_theta in [-pi, pi]; the Jacobian
 *                                                                       with respect to the pose is the identity
 *   chi2 = max(0, d' Lambda d),   cost term 1/2 rho(chi2)
 * with rho ONE pgo_loss for all priors of the handle (NULL = Trivial), evaluated by the function of csrc/loss.h, and the
 * corrector the sqrt(rho') row scaling every loss here uses.  With S_i the Jacobi scales of pose i the scaled system gains
 * hd_i += rho' S_i Lambda S_i and gs_i += rho' S_i Lambda d.  A constant pose has zero scale: it receives exactly nothing, but
 * its prior still counts in the cost.  Lambda is symmetric, given as I11 I12 I13 I22 I23 I33 (the order of the edges'
 * information), finite and positive SEMI-definite: diag(a, a, 0), a position-only fix, is legal and the common case.  The
 * rounding allowance: the smallest eigenvalue may be as low as -1e-12 x the largest absolute eigenvalue (what forming Q Omega Q'
 * in floating point leaves of an exact zero); a prior whose smallest eigenvalue is above +1e-12 x the largest is positive
 * definite and counts as a gauge for the calls that refuse an unanchored problem (pgo_pose_covariance and the gates).  At most
 * one prior per pose.
 * - pgo_set_priors: n priors on the poses pose[k] (the caller's numbering); n = 0 clears them (the arrays are not read), and a
 *   pgo_solve after clearing gives bitwise what a fresh handle gives.  Each call replaces the whole set.  A handle with priors
 *   keeps whatever K1 instantiation it had: priors never touch K1, and a handle without priors launches neither of their kernels.
 * - pgo_eval's cost, the LM loop (pgo_solve, pgo_lm_step), pgo_iter_record.cost and the gradient norm include the priors, and so
 *   do pgo_gnc_solve and pgo_mixture_solve, which go through the LM loop.  pgo_eval's r and J outputs stay the EDGES' rows;
 *   pgo_debug_normal_eq returns the system with the priors.  info_weighting = 1 is supported: the priors are independent of K1's
 *   whitening.
 * - pgo_pose_covariance, pgo_edge_gate and pgo_edge_gate_joint (both `solver` settings) see the problem WITH priors.  A positive
 *   definite prior on a pose that is free at the time of the call is a gauge for them (pgo_set_active may free or fix the pose
 *   later, in either order).  solver = 1 runs on handles on the direct solve, and those have a constant pose (below): with
 *   solver = 1 the priors are only ever met NEXT to a hard anchor, never as the only gauge.
 * - pgo_edge_weights, pgo_edge_chi2, pgo_loop_support, pgo_chordal_init, pgo_coarsen* and pgo_prolong do not know priors: they
 *   report on, or start from, the edges alone.
 * - pgo_set_losses, pgo_set_active and pgo_set_edge_weights leave the priors alone, in either call order.  A solve begun with
 *   pgo_lm_begin becomes stale: pgo_lm_step returns PGO_ERR_INVALID_ARG until pgo_lm_begin runs again, as after pgo_set_losses.
 * - The direct solve (linear_solver 2) adds the priors' blocks to the diagonal of its chain matrix T, which stays a sum of
 *   positive semi-definite terms.  The solver of a handle is planned at pgo_create*, before any prior exists, and that plan
 *   keeps its rule: the direct solve needs a constant pose (fixed_pose >= 0), so a handle whose gauge comes from priors alone
 *   (fixed_pose = -1) solves by PCG, and linear_solver = 2 stays PGO_ERR_UNSUPPORTED for it.  Priors only add to T's
 *   diagonal; a direct solve that fails all the same is redone by PCG as ever (pgo_handle_info.direct_fallbacks).
 * - pgo_window_solve returns PGO_ERR_UNSUPPORTED while priors are set (its kernel evaluates its own system).  There is no batch
 *   entry point.
 * - pgo_get_prior_residuals: d (n x 3) and chi2 (n) of the plain residual at the handle's poses (or at poses_or_null, N x 3 in
 *   the caller's order), in the order the priors were given; runs on the GPU.  Either output may be NULL.
 * - pgo_prior_eval: the host evaluation of the same header -- d, chi2 and rho[0..2] = rho, rho', rho'' at chi2.
 * Errors (nothing changes on error): PGO_ERR_INVALID_ARG for a null handle or a null array with n > 0, n < 0, a pose out of range
 * or a duplicate pose (pgo_last_error names the first), a mean or information that is not finite, an information with a negative
 * eigenvalue beyond the allowance, an invalid loss; PGO_ERR_UNSUPPORTED for METHOD 2, a communicator or
 * PGO_FORCE_COLLECTIVES=1, a batched handle.                                                                                   */
int     pgo_set_priors(pgo_t* h, int32_t n, const int32_t* pose, const double* mean_xyt /* n x 3 */, const double* info6 /* n x 6 */,
                       const pgo_loss* loss_or_null);                                                                  /* [gpu] */
int32_t pgo_num_priors(const pgo_t* h);                                                                                /* [host] */
int     pgo_get_prior_residuals(pgo_t* h, const double* poses_or_null, double* d_out /* n x 3 */, double* chi2_out /* n */);  /* [gpu] */
int     pgo_prior_eval(const double pose[3], const double mean[3], const double info6[6], const pgo_loss* loss_or_null, double d[3],
                       double* chi2, double rho[3]);                                                                   /* [host] */

/* ------------------------------------------------ kernel-level entry points
 * Used by the parity tests and by bench.py's roofline leg: each launches exactly
 * one kind of kernel `reps` times on the handle's stream, brackets the launches
 * with HIP events on that stream and returns the average milliseconds.          */
typedef struct pgo_kernel_stats {
  double ms_avg;              /* average launch duration (HIP events)            */
  double algorithmic_bytes;   /* bytes one launch must move    */
  int64_t units;              /* edges (K1/K2) or blocks (K3) per launch         */
} pgo_kernel_stats;
int pgo_bench_eval(pgo_t* h, int reps, int with_jacobian, pgo_kernel_stats* out); /* [gpu] K1 */
int pgo_bench_assemble(pgo_t* h, int reps, pgo_kernel_stats* out);                /* [gpu] K2 */
int pgo_bench_spmv(pgo_t* h, int reps, pgo_kernel_stats* out);                    /* [gpu] K3 */
/* z = M^-1 r with the preconditioner the next LM iteration applies: current linearisation, current radius (both entry
 * points first set up the LM diagonal and the preconditioner, as an LM iteration does; the solve itself is not affected).
 * Needs at least one LM iteration.  r, z: 3N doubles, caller's pose order.  world == 1, or several ranks with the second
 * preconditioner level on: then a collective call -- every rank passes the whole r and receives z on the rows it owns
 * (0 on the others), so that the ranks' z add up to the applied M^-1 r.                                               */
int pgo_debug_precond(pgo_t* h, const double* r_3n, double* z_3n);               /* [gpu] */
int pgo_bench_precond(pgo_t* h, int reps, pgo_kernel_stats* out);                 /* [gpu] z = M^-1 b as the PCG start-up kernel */
/* y = (J'J) x in the scaled space at the current linearisation, WITHOUT the LM diagonal; x,y: 3N doubles (world == 1).
 * For SpMV parity tests.                                                                                              */
int pgo_debug_spmv(pgo_t* h, const double* x, double* y);                         /* [gpu] */
/* y = (J'J + D'D) x through the product kernel the PCG loop runs, after the same set-up as pgo_debug_precond (LM diagonal
 * for the current radius); optionally d2 = the diagonal of D'D (3N).  x, y, d2: caller's pose order (world == 1).     */
int pgo_debug_system_spmv(pgo_t* h, const double* x, double* y, double* d2_or_null);   /* [gpu] */
/* y = (J'J + D'D)^-1 b by the handle's direct solve (chain + low rank) at its current LM state, through the launch sequence
 * an LM iteration runs; b, y: 3N doubles in the conventions of pgo_debug_system_spmv, whose product of y gives b back.  The
 * rows of the constant pose must be 0 in b, as they are in LM's gradient.  refine_steps: -1 = the handle's own number of
 * iterative-refinement steps (what LM runs), 0 = the raw Woodbury result, 1 .. 3 = that many.  The solve is not affected.
 * METHOD 2 after a rejected step: the reduced pose system is the one assembled for the previous radius until the next LM
 * iteration re-assembles it; this entry point and pgo_debug_system_spmv both see that one.
 * PGO_ERR_UNSUPPORTED on a handle that is not on the direct solve (pgo_handle_info.linear_solver), PGO_ERR_INVALID_ARG
 * for a null pointer, refine_steps outside -1 .. 3 or a handle without pgo_lm_begin.                                    */
int pgo_debug_direct_solve(pgo_t* h, const double* b_3n, int32_t refine_steps, double* y_3n);   /* [gpu] */
/* The linear solve of ONE LM iteration of every problem of a batch, through the launch a pgo_batch_solve iteration runs (one
 * workgroup per problem), at the batch's current poses: the set-up of the solve's start (unit scales, Jacobi scales from this
 * Jacobian), `radius` for every problem, at most max_it PCG iterations to |r| <= rtol |b| for every problem, all of them active.
 * rhs, y_out: the problems' unknowns concatenated in problem order, 3 n_k doubles each in each problem's own pose numbering,
 * scaled space (the conventions of pgo_debug_system_spmv); rhs == NULL: the scaled gradient, as LM solves.  The rows of each
 * problem's constant pose must be 0 in rhs.  res[k]: the PCG state of problem k at exit and the sums of the step's epilogue
 * (y.b, y.(H y) without the LM diagonal, |S y|^2).  Poses, per-problem LM state, records, losses / weights / active set are
 * untouched: a pgo_batch_solve afterwards returns bitwise what it returns without the call.
 * PGO_ERR_INVALID_ARG: a null b / y_out / res, radius not finite or <= 0, max_it outside 0 .. 1000000, rtol negative or not finite. */
typedef struct pgo_solo_result { double rz, bb, rr, ydotg, yHy, step2; int32_t iters, done; } pgo_solo_result;
int pgo_batch_debug_solve(pgo_batch_t* b, double radius, int32_t max_it, double rtol,
                          const double* rhs_or_null, double* y_out, pgo_solo_result* res /* n */);   /* [gpu] */
/* normal-equation pieces at the current point, caller's pose order (world == 1):
 * g: 3N gradient J'r (unscaled), hdiag: N x 9 diagonal 3x3 blocks of J'J; 0 on the constant pose.  The call re-evaluates the
 * residuals at the current poses, resets the pose scales to 1 and ends the solve begun with pgo_lm_begin.
 * METHOD 2: the REDUCED pose system, not the joint one -- g = P'(r - gamma j) and the diagonal blocks of P'(I - c j j')P, P the
 * pose columns of the Jacobian at the current poses and switches, j = d e / d s per robust edge, with the c and gamma of the
 * handle's last assembly (k_switch_prepare: the switches eliminated for the radius of that assembly, their Jacobi scales kept). */
int pgo_debug_normal_eq(pgo_t* h, double* g_or_null, double* hdiag_or_null);      /* [gpu] */
/* Test hooks -- for tests/ only, not part of the drop-in surface.  Process-wide knobs read by pgo_create* (handles
 * created afterwards); value < 0 restores the library's default.  The library reads NO environment variable other than
 * PGO_FORCE_COLLECTIVES (1 = issue the collectives at world == 1 too, where they are identities) and
 * PGO_GRAPH_COLLECTIVES (0 = never capture collectives into the PCG hipGraph, 1 = all-reduce / all-gather, 2 = also the
 * point-to-point exchange), and never lets the environment override a pgo_options field.
 *   "spmv_pipe"          0 = K3 as k_spmv_t; 2 = K3 as the software-pipelined k_spmv_p even where k_spmv_1 (one row tile
 *                        per workgroup, graphs with more than 4096 tiles) is the default (all three must agree)
 *   "fused_p"            0 = small graphs keep the three-launch PCG loop (no direction update inside the SpMV)
 *   "direct_fail_at"     k = the direct solve of LM iteration k returns NaNs (exercises the PCG redo)
 *   "direct_setup_fail"  1 = setting up the direct solver fails with PGO_ERR_NOMEM after its first allocations
 *   "single_reduction"   1 / 0 = force the one-reduction (Chronopoulos-Gear) PCG loop on / off (default: on for
 *                        world > 1 in the inexact mode, pcg_rtol >= 1e-6)
 *   "verify_residual"    1 = pcg_rel_residual of the iteration records is the TRUE |b - A y| / |b| of each PCG solve (one
 *                        more product per solve) instead of the recurrence residual the loop stopped on
 *   "shm_timeout_s"      seconds a rank of the shm TEST communicator waits at a barrier before it gives up (default 120)
 *   "pad_tiles"          0 = large graphs keep the dense incidence layout (default: every row tile padded to 256 incidence
 *                        slots of its own, so that K3 finds a tile's blocks from its number alone; same results);
 *                        1 = that layout and its product kernel (k_spmv_1) on a graph of any size
 *   "cov_poses_per_pass" 1..16 = overrides pgo_covariance_options.poses_per_pass of every pgo_pose_covariance / pgo_edge_gate call (read per call;
 *                        the results agree with every value up to the solver tolerance)
 *   "cov_direct_cols"    a multiple of 3 in 3..768 = columns per pass of pgo_pose_covariance / pgo_edge_gate with solver = 1 (read per
 *                        call; any other value >= 0: PGO_ERR_INVALID_ARG from that call; the results are bitwise the same for every width);
 *                        pgo_posterior_sample with solver = 1 draws that many samples per pass
 *   "gate_joint_shape"   0 = pgo_edge_gate_joint runs its elimination as ONE launch of one workgroup instead of one launch per
 *                        candidate with a grid of workgroups over the trailing rows (read per call; the results are bitwise the same)
 *   "score_grid"         n > 0 = pgo_trajectory_error launches n workgroups over its chunks instead of one per chunk (read per
 *                        call; the results are bitwise the same)
 *   "coarsen_grid"       n > 0 = pgo_coarsen and pgo_prolong launch n workgroups over their segments, chunks and poses instead of
 *                        one per unit of work (read per call; the results are bitwise the same)
 *   "gnc_grid"           n > 0 = pgo_gnc_update (and pgo_gnc_solve through it) launches n workgroups over its chunks of 256 edges
 *                        instead of one per chunk (read per call; the results are bitwise the same)
 *   "support_grid"       n > 0 = pgo_loop_support launches n workgroups over its segments, poses, loops and chunks of 256 edges
 *                        instead of one per unit of work (read per call; the trajectory is computed at a handle's first call; the
 *                        results are bitwise the same)
 *   "chordal_grid"       n > 0 = pgo_chordal_init launches n workgroups over its tiles of 256 rows and chunks of 256 edges instead
 *                        of one per unit of work (read per call; the results are bitwise the same)
 *   "mix_grid"           n > 0 = pgo_mixture_select (and pgo_mixture_solve through it) launches n workgroups over its chunks of
 *                        256 mixture edges (read per call; the results are bitwise the same)
 *   "prior_add_grid"     n > 0 = k_prior_add, which adds the pose priors to the assembled system, launches n workgroups over its
 *                        chunks of 256 priors (read per launch; the results are bitwise the same)
 * Unknown name: PGO_ERR_INVALID_ARG.                                                                     */
int pgo_debug_set_knob(const char* name, long long value);                        /* [host] */
/* sharding plan of a graph over `world` ranks: for rank r, rows [lo, hi) and the
 * number of local edges / cut edges.  rows per rank = ceil(N / world) rounded up to a
 * multiple of row_align (the solver passes its preconditioner block size, see
 * pgo_options.pcg_block_poses; 1 = plain ceil).  Pure host logic.                */
int pgo_shard_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib,
                   int world, int rank, int row_align, int32_t* lo, int32_t* hi,
                   int32_t* n_local_edges, int32_t* n_cut_edges);                 /* [host] */
/* Locality ordering of the poses, the permutation the solver applies internally when pose_ordering = 1:
 * perm[i] = new position of pose i.  Segments of `segment` consecutive poses stay contiguous and in order (the
 * odometry chain and the preconditioner's pose blocks survive; `segment` should be a multiple of the block size);
 * the segments are reordered by reverse Cuthill-McKee on the graph of SUPPORTED loop edges -- (a, b) is supported
 * when some edge joins {a-1, a, a+1} x {b-1, b, b+1} other than itself, which keeps the mesh of true revisits and drops
 * isolated random loops; the last (short) segment stays last.  Pure host logic.                                     */
int pgo_pose_order(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, int32_t segment,
                   int32_t* perm);                                                /* [host] */
/* halo of that plan: send_rows[s] = how many of rank's rows peer s references, recv_rows[s] = how many of
 * peer s's rows rank references (arrays of `world` entries; the own-rank entries are 0).  Pure host logic.  */
int pgo_shard_halo(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib,
                   int world, int rank, int row_align, int64_t* send_rows, int64_t* recv_rows); /* [host] */

#ifdef __cplusplus
}
#endif
#endif /* PGO_H_ */
