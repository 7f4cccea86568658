/*
 * lfvio_debug.h — parity / inspection hooks of liblfvio_hip.so used by tests/, tools/ and bench.py only.
 * Not part of the drop-in boundary (include/lfvio.h).  Ten entry points: two that take a key, eight that look inside.
 */
#ifndef LFVIO_DEBUG_H
#define LFVIO_DEBUG_H
#include "lfvio.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Every switch of the library in one call.  LFVIO_ERR_ARG for an unknown key or a value out of range.
 *   "graph"              0: launch kernels directly, 1 (default): replay the captured hipGraphs
 *   "first_passes"       n > 0: every first graph of the synchronous entry points carries n passes instead of the most any of the last
 *                        four calls needed; 0: adaptive again
 *   "spec_count"         n > 0: a fixed number of speculative candidates per pass (1 .. 4); 0: from the call before (3, or 4).  The
 *                        answer of a call — state, inverse depths, summary, trace, prior — is the same bytes for every value, and so
 *                        for every history of a context (tests/test_spec_candidates.py); only the passes a call takes differ
 *   "function_tolerance" Solver::Options::function_tolerance of the windows uploaded from now on (Ceres' default 1e-6, which
 *                        estimator.cpp:810-822 leaves alone); 0 makes the loop run to its iteration cap or another criterion
 *   "initial_radius"     Solver::Options::initial_trust_region_radius of the windows uploaded from now on (Ceres' default 1e4; <= 0
 *                        restores it).  A small radius takes the dogleg through its Cauchy-point and interpolation cases at once
 *   "linw"               where the strip sweep (kernels_linw.h) replaces the role-by-role one (k_lin + k_sum): 1 (default) for a resident
 *                        batch whose windows all carry a plan (k_linw) and for a single window — or a rank's share — of at least 40 960
 *                        landmarks (k_linb + k_sumb); 0 never; 2 for every launch, however few or small the windows (tests).  With the
 *                        next upload
 *   "lm_half"            1 (default): the landmark role of k_lin runs eight lanes per track, 32 landmarks per workgroup, for windows of
 *                        at most 320 landmarks uploaded from now on; 0: four lanes, 64 landmarks, the form larger windows take
 *   "force_eig"          != 0: the pseudo-inverse of the marginalization's dropped block always from its eigen-decomposition
 *                        (marginalization_factor.cpp:267-272); default: from a Cholesky factorization when every eigenvalue is provably
 *                        far above eps
 *   "marg_ahead"         0: the windows uploaded from now on end with the serial tail (gauge fix, frame-0 sweep, k_marg_solve behind the
 *                        last pass); 1 (default): a one-window context of at most 320 landmarks starts the marginalization of every
 *                        newly accepted state on worker streams (csrc/kernels_spec.h).  Either way the prior is the same bits
 *   "break_next_chain"   1: the next lfvio_batch_upload_chained_device promises the device a prior of one row more than the
 *                        marginalization in flight will leave — the path a failed marginalization takes, for tests
 *   "relo_route"         1: lfvio_solve_relo takes its own route (kernels_relo.h) also without a match, instead of lfvio_solve; 0 (default)
 *   "env"                apply LFVIO_DEBUG="key=value,key=value" from the environment (the product entry points read none) */
int lfvio_debug_configure(lfvio_ctx *ctx, const char *key, double value);
/* What the last calls left, as doubles into out[0 .. n).
 *   "last_call"     {passes of the trust-region loop the slowest window of the last synchronous call used, iterations they covered,
 *                   graph launches of that call (1: everything ran in the first graph), speculative candidates per pass: the fixed number, or what the
 *                   last call that speculated chose from the two counts of the call before it}
 *   "marg_ahead"    {calls that started workers, priors a worker delivered} since the context was created
 *   "upload_times"  microseconds of the last upload: host packing | collecting a chained prior | prior + copies enqueued | final wait
 *   "sweep_kernel"  in out[0]: a count of resident slots; out[0]: the kernel that linearizes a launch over them — 0 k_lin (+ k_sum),
 *                   1 k_linw (a resident batch), 2 k_linb (+ k_sumb: a large single window); out[1] (n >= 2): 1 where k_lin goes out
 *                   role by role (k_lin<LIN_ROLE_LM>, <LIN_ROLE_GRAM>, k_imu_raw + k_lin<LIN_ROLE_POSE_RAW>), 0 where it is one grid */
int lfvio_debug_query(lfvio_ctx *ctx, const char *key, double *out, int n);
/* Gauss-Newton blocks at the window's state, caller landmark order:
 * Hpp 172x172 row-major, gp 172, a/b N, W N x 73, cost. */
int lfvio_debug_linearize(lfvio_ctx *ctx, const LfvioWindow *in, double *Hpp, double *gp, double *a, double *b,
                          double *W, double *cost);
/* The Schur sums of a solve repeated with a new mu on the stored linearization (do_schur without do_lin) against a
 * full re-linearization at the same mu: largest absolute difference (expected 0). */
int lfvio_debug_schur_repeat(lfvio_ctx *ctx, const LfvioWindow *in, double mu, double *max_abs_diff);
/* Post-Schur system (A' n x n, b' n) of the last marginalization run on slot 0 by the loop's own stream. */
int lfvio_debug_marg_system(lfvio_ctx *ctx, int n, double *A, double *b);
/* shader-clock stamps written by the profiling builds of the kernels of slot 0 (bring-up instrumentation) */
int lfvio_debug_read_clocks(lfvio_ctx *ctx, long long *out32);
/* Average ms of `reps` launches of one pipeline kernel over slots [0,count) (HIP events on the context stream).
 * which: 0 k_lin (residual/Jacobian sweep + Schur SYRK of the landmark blocks), 2 k_sum (+ k_presum), 3 k_solve_dense;
 * 4 .. 7 k_setup by role, 8 .. 10 k_lin by role; a resident batch on the strip sweep: 12 k_linw, 13 k_solve_dense<true>, 14 k_stepw;
 * a large window group by group: 15 k_linb, 16 k_sumb, 17 k_backsub_wt (an error where the launch does not take that path). */
int lfvio_debug_time_kernel(lfvio_ctx *ctx, int which, int count, int reps, double *avg_ms);
/* What the dense solve (k_solve_dense, csrc/kernels_solve.h) read and what it wrote, for tests/test_solve_hp.py.  One linearization +
 * dense solve of the resident slots [0, count) from their uploaded state, by the path the launch takes — k_setup, the sweep and the solve
 * of the launch's own route; with mu > 0, tr.mu of every slot's header is set to it between k_setup and the sweep (mu <= 0: the 1e-8
 * k_setup leaves) — adds no kernel and no kernel argument, and copies down memory the pass leaves in slot `slot`.  Every pointer of `io`
 * may be NULL.  Returns the sweep kernel: 1 if k_linw ran, 2 if k_linb + k_sumb, 0 if k_lin + k_sum; < 0 on error.
 *   read by the solve    H        the H region of the exchange buffer, 14 878 packed doubles (lower triangle, entry (i, j <= i) at
 *                                 i (i + 1) / 2 + j): complete H_pp behind k_sum / k_sumb; behind k_linw only the visual terms of the camera
 *                                 rows (i < 73), the rest of it is whatever an earlier pass left
 *                        gp[172], schur[15 x 256] (tile layout), lm_sum[16], imu_out[10 x 932] (per factor: its 30 x 30 block over
 *                        [pose_f | sb_f | pose_f+1 | sb_f+1] row-major — behind k_linw only the entries whose tangent row is not above
 *                        their tangent column, the ones the solve takes — 30 gradient entries, the cost), prior_A[prior_n x prior_n] (room
 *                        for 172 x 172), prior_cmap[172] (prior column -> tangent column)
 *   read by the sweep's Schur phase   a[N], b[N], W[N x 73]: device landmark order, W unpacked from the rows the route leaves
 *                        (the compact rows behind k_lin, the transposed ones behind k_linw / k_linb) over each landmark's span
 *   written by the solve scale_p, diag_p, grad_p, gn_p [172 each], uc_grad, uc_gn [80 each: 73 entries and the zero padding], q[16]
 *   scalars, always filled in: the trust-region header after the pass and the sizes the arrays above go with */
typedef struct LfvioPassIO {
  double *H, *gp, *schur, *lm_sum, *imu_out, *prior_A;
  int *prior_cmap;
  double *a, *b, *W;
  double *scale_p, *diag_p, *grad_p, *gn_p, *uc_grad, *uc_gn, *q;
  double alpha, grad_sq_total, x_cost, mu, prior_cost; /* tr.alpha, tr.grad_sq_total, tr.x_cost, tr.mu; prior_g[172], the prior's cost */
  int chol_fail, prior_n, est_ex, est_td, num_landmarks;
} LfvioPassIO;
int lfvio_debug_pass_io(lfvio_ctx *ctx, int count, int slot, double mu, LfvioPassIO *io);
/* The step half of the same pass — landmark back-substitution, dogleg, candidates, their cost at every factor, bookkeeping — for
 * tests/test_step_hp.py.  Launches exactly what lfvio_debug_pass_io launches (mu > 0 replaces tr.mu and radius > 0 tr.radius of every slot
 * between k_setup and the sweep), then the step half through the very function the loop's passes go through, by the route that launch takes:
 * k_step | k_backsub / k_backsub_wt + k_dogleg + k_cost (+ k_cost_imu) + k_decide | k_stepw.  `spec`: candidates per pass, 1 .. 4 where the
 * route speculates (here: count = 1 and at most 320 landmarks), 1 otherwise (LFVIO_ERR_ARG if not).  The bookkeeping is k_decide, the form behind
 * the last pass of a sequence, except in k_stepw, which carries it.  Adds no kernel and no kernel argument.  On the routes with a k_decide of
 * their own the stream is joined in front of it and `head`, the candidates and their sums are copied then (head_valid 1); behind k_stepw
 * `head` is the header in front of the step half, with the totals the step half wrote (gn_sq_total, grad_gn_total, gmax_pose, spec_n) taken
 * from the copy after it, as the candidates are: its bookkeeping leaves them alone (head_valid 0).  Every pointer may be NULL.  Returns the sweep kernel as lfvio_debug_pass_io does, < 0 on error.
 *   LFVIO_STATE_DOUBLES   a state: pose [11][7] | speed/bias [11][9] | ex [7] | td
 *   read by the step half   pass: everything of LfvioPassIO; scale_l, diag_l, grad_l, einv_l, lam [N] (device landmark order; lam = lam[cur]),
 *                           x [LFVIO_STATE_DOUBLES] = x[cur], head: the header in front of the bookkeeping
 *   written                 gn_l, d1, d2 [N], step_p [172]; per candidate z < spec (slot z of every array): coef [4][5] = cg, cn,
 *                           dogleg_step_norm, step_sq_pose, xn2_pose_cand; cand_x [4][LFVIO_STATE_DOUBLES]; cand_lam [4][N]; block_sums
 *                           [4][num_blocks][5] = cost, mlin, mquad, dn, xn of every landmark block (behind k_stepw the window's totals in
 *                           block 0); pose_cost [4][11]: IMU factors 0 .. 9 and the prior; cand_tab [4][tab_bytes]: the pair table
 *   after the bookkeeping   after (the header), trace [LFVIO_MAX_TRACE] (entries head.trace_len .. after.trace_len - 1 are this pass's),
 *                           x_after, lam_after [N], tab_after [tab_bytes]: x / lam / tab [after.cur] */
#define LFVIO_STATE_DOUBLES (11 * 7 + 11 * 9 + 7 + 1)
typedef struct LfvioStepHeader {
  double radius, mu, x_cost, x_norm, cand_cost, model_cost_change, alpha, grad_sq_total, gn_sq_total, grad_gn_total, gmax_pose, function_tolerance;
  double q[16];
  int iteration, cur, do_lin, do_schur, done, termination, chol_fail, num_succ, num_unsucc, consec_invalid, trace_len, skip_step, spec_n, max_iter;
} LfvioStepHeader;
typedef struct LfvioStepIO {
  LfvioPassIO pass;
  double *scale_l, *diag_l, *grad_l, *einv_l, *lam, *x;
  double *gn_l, *d1, *d2, *step_p;
  double *coef, *cand_x, *cand_lam, *block_sums, *pose_cost;
  unsigned char *cand_tab, *tab_after;
  double *x_after, *lam_after;
  LfvioIterationSummary *trace;
  LfvioStepHeader head, after;
  int head_valid, num_blocks, tab_bytes, spec, stepw; /* head was copied in front of the bookkeeping | landmark blocks | sizeof the pair table | candidates | 1: k_stepw ran */
} LfvioStepIO;
int lfvio_debug_step_io(lfvio_ctx *ctx, int count, int slot, double mu, double radius, int spec, LfvioStepIO *io);
/* tests: the local context `local_ctx` of the group reports a failure when it enqueues phase `phase` (0 the sweep, 4 solve ..
 * candidate cost, 3 bookkeeping) of pass `pass` of the next lfvio_group_optimize(); local_ctx < 0 clears it.
 * The call must still issue every collective of its sequence (the peers of a real group are waiting in them), end the loops of all
 * ranks in the same pass and return the error. */
int lfvio_debug_group_inject_failure(lfvio_group *g, int local_ctx, int pass, int phase);
#ifdef __cplusplus
}
#endif
#endif
