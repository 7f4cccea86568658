/*
 * lfvio.h — C-ABI boundary of the MI355X sliding-window solver.
 *
 * This is the single host -> device seam of the drop-in.  The reference has no
 * FFI: its seam is the C++ member `void Estimator::optimization()`
 * (vins_estimator/src/estimator.h:47, body estimator.cpp:676-1009), which talks
 * to Ceres through flat `para_*` arrays (estimator.h:107-113) filled by
 * `vector2double()` (estimator.cpp:488-530).  A re-implemented
 * `optimization()` body packs exactly those arrays, the feature-per-frame
 * observations (feature_manager.h:18-71), the ten `IntegrationBase` results
 * (factor/integration_base.h:188-203) and the marginalization prior
 * (factor/marginalization_factor.h:47-72) into the PODs below and calls the
 * entry points declared here.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - everything is FP64; matrices are ROW-major; quaternions inside pose
 *     blocks are stored [x y z w] exactly like para_Pose (estimator.cpp:492-499);
 *     preintegration delta_q is [x y z w] (Eigen coeffs() order).
 *   - pose block  = [px py pz qx qy qz qw]                  (SIZE_POSE = 7)
 *     speed/bias  = [vx vy vz bax bay baz bgx bgy bgz]      (SIZE_SPEEDBIAS = 9)
 *   - caller owns every buffer; the context owns device memory, streams and
 *     graphs; no pointer is retained across calls.
 *   - every function returns LFVIO_OK (0) or a negative error; on error the
 *     outputs are untouched so the caller can fall back (the reference itself
 *     has no error channel: optimization() is void, estimator.cpp:676).
 *   - one caller at a time per context (the reference holds m_estimator across
 *     processImage(), estimator_node.cpp:215-332).
 */
#ifndef LFVIO_H
#define LFVIO_H

#ifdef __cplusplus
extern "C" {
#endif

#define LFVIO_WINDOW_SIZE 10                      /* parameters.h:12 */
#define LFVIO_NUM_FRAMES (LFVIO_WINDOW_SIZE + 1)  /* estimator.h:107 */
#define LFVIO_SIZE_POSE 7                         /* parameters.h:45 */
#define LFVIO_SIZE_SPEEDBIAS 9                    /* parameters.h:46 */
#define LFVIO_MAX_PRIOR_BLOCKS 24                 /* 11 poses + 11 speed/bias + ex + td */
#define LFVIO_MAX_PRIOR_DIM 172                   /* 11*6 + 11*9 + 6 + 1 tangent dims */
#define LFVIO_MAX_TRACE 64

/* error codes */
#define LFVIO_OK 0
#define LFVIO_ERR_ARG (-1)         /* malformed window (bad CSR, NULL, sizes)  */
#define LFVIO_ERR_DEVICE (-2)      /* HIP runtime error                         */
#define LFVIO_ERR_NONFINITE (-3)   /* non-finite cost / state / prior           */
/* A reduced system that never becomes positive definite is NOT an error of the call: as in Ceres, every failed
 * factorization is an invalid step (mu *= 10), five in a row end the solve with termination = LFVIO_FAILURE and the
 * state of the last accepted step (trust_region_minimizer.cc: HandleInvalidStep). */

/* marginalization flags: Estimator::MarginalizationFlag, estimator.h:58-62 */
#define LFVIO_MARGIN_OLD 0
#define LFVIO_MARGIN_SECOND_NEW 1

/* termination: ceres::TerminationType subset used by TrustRegionMinimizer */
#define LFVIO_CONVERGENCE 0
#define LFVIO_NO_CONVERGENCE 1
#define LFVIO_FAILURE 2

/* parameter-block identity.  The reference identifies prior blocks by the
 * ADDRESS of para_* rows (addr_shift, estimator.cpp:921-933); the ABI uses
 * (kind, frame) tags instead. */
#define LFVIO_BLOCK_POSE 0       /* para_Pose[frame],       global 7 / local 6 */
#define LFVIO_BLOCK_SPEEDBIAS 1  /* para_SpeedBias[frame],  9 / 9              */
#define LFVIO_BLOCK_EX_POSE 2    /* para_Ex_Pose[0],        7 / 6              */
#define LFVIO_BLOCK_TD 3         /* para_Td[0],             1 / 1              */

typedef struct LfvioBlockId {
  int kind;
  int frame;
} LfvioBlockId;

/* One IntegrationBase (factor/integration_base.h:188-203) as consumed by
 * IMUFactor::Evaluate (factor/imu_factor.h:19-200). */
typedef struct LfvioPreintegration {
  double sum_dt;
  double delta_p[3];
  double delta_q[4]; /* x y z w */
  double delta_v[3];
  double linearized_ba[3];
  double linearized_bg[3];
  double jacobian[225];   /* 15x15 row-major, order O_P O_R O_V O_BA O_BG */
  double covariance[225]; /* 15x15 row-major */
} LfvioPreintegration;

/* MarginalizationInfo after marginalize()+getParameterBlocks()
 * (factor/marginalization_factor.cpp:174-319): the kept blocks in order,
 * their linearization points, and linearized_jacobians / linearized_residuals. */
typedef struct LfvioPrior {
  int valid;      /* 0 => no prior (last_marginalization_info == nullptr) */
  int m;          /* marginalized tangent dim (informational)             */
  int n;          /* kept tangent dim = rows = cols of linearized_jacobians */
  int num_blocks; /* kept parameter blocks                                 */
  LfvioBlockId blocks[LFVIO_MAX_PRIOR_BLOCKS]; /* AFTER addr_shift          */
  int block_idx[LFVIO_MAX_PRIOR_BLOCKS];       /* column offset (keep_block_idx - m) */
  double block_x0[LFVIO_MAX_PRIOR_BLOCKS][9];  /* keep_block_data (global size) */
  double linearized_jacobians[LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM]; /* n x n row-major, leading dim n */
  double linearized_residuals[LFVIO_MAX_PRIOR_DIM];
} LfvioPrior;

/* The whole input of one optimization() call. */
typedef struct LfvioWindow {
  /* state, as written by vector2double() (estimator.cpp:488-530) */
  double para_pose[LFVIO_NUM_FRAMES][LFVIO_SIZE_POSE];
  double para_speed_bias[LFVIO_NUM_FRAMES][LFVIO_SIZE_SPEEDBIAS];
  double para_ex_pose[LFVIO_SIZE_POSE];
  double para_td;

  /* flags / solver options (estimator.cpp:690-703, 810-822) */
  int estimate_extrinsic;            /* ESTIMATE_EXTRINSIC != 0                */
  int estimate_td;                   /* ESTIMATE_TD: ProjectionTdFactor vs ProjectionFactor */
  int max_num_iterations;            /* NUM_ITERATIONS                          */
  double max_solver_time_in_seconds; /* <= 0: disabled (parity / bench runs); > 0: honoured by the synchronous entry
                                        points between graph launches (every 2 passes), ignored by *_async    */

  /* globals read by the factors (parameters.h:17-41) */
  double g[3];      /* G                                      */
  double tr;        /* TR (rolling-shutter read-out time)     */
  double row;       /* ROW (image height)                     */
  double sqrt_info; /* FOCAL_LENGTH / 1.5, estimator.cpp:18-19 */

  /* landmarks that pass `used_num >= 2 && start_frame < WINDOW_SIZE - 2`
   * (feature_manager.cpp:36), in f_manager.feature list order, CSR over
   * their feature_per_frame vectors.  Observation o of landmark l is seen in
   * frame start_frame[l] + (o - obs_offset[l]); the first one is the anchor
   * (estimator.cpp:737-745). */
  int num_landmarks;
  int num_observations;            /* obs_offset[num_landmarks]              */
  const int *start_frame;          /* [N]                                    */
  const int *obs_offset;           /* [N+1]                                  */
  const double *inv_depth;         /* [N] para_Feature = 1/estimated_depth   */
  const double *obs_point;         /* [M][3] FeaturePerFrame::point (unit bearing) */
  const double *obs_velocity;      /* [M][3] FeaturePerFrame::velocity       */
  const double *obs_cur_td;        /* [M]    FeaturePerFrame::cur_td         */
  const double *obs_uv_y;          /* [M]    FeaturePerFrame::uv.y()         */

  /* pre_integrations[1..10] (estimator.cpp:717-724); imu[i] links frame i -> i+1 */
  LfvioPreintegration imu[LFVIO_WINDOW_SIZE];

  /* last_marginalization_info (+ parameter blocks); prior->valid==0 or NULL => none */
  const LfvioPrior *prior;
} LfvioWindow;

typedef struct LfvioIterationSummary { /* ceres::IterationSummary subset */
  double cost;
  double cost_change;
  double gradient_max_norm; /* NaN in the entry of a successful iteration that ended the loop (iteration cap, wall-clock cap): Ceres
                             * evaluates the gradient at the accepted point before it tests the cap, the device's next
                             * linearization never happens; the reference reads no summary field.  lfvio_debug_linearize() at the
                             * solution gives it (tests/test_gpu_parity.py::test_kkt_residual_at_the_solution). */
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  int step_is_valid;
  int step_is_successful;
} LfvioIterationSummary;

/* Output of the solve: the para_* arrays as Ceres leaves them (BEFORE
 * double2vector(), estimator.cpp:830, which stays on the host). */
typedef struct LfvioSolution {
  double para_pose[LFVIO_NUM_FRAMES][LFVIO_SIZE_POSE];
  double para_speed_bias[LFVIO_NUM_FRAMES][LFVIO_SIZE_SPEEDBIAS];
  double para_ex_pose[LFVIO_SIZE_POSE];
  double para_td;
  double *inv_depth; /* [N] caller-allocated */
  int num_iterations; /* summary.iterations.size() (iteration 0 included) */
  int num_successful_steps;
  int num_unsuccessful_steps;
  int termination;
  double initial_cost;
  double final_cost;
  LfvioIterationSummary trace[LFVIO_MAX_TRACE];
} LfvioSolution;

typedef struct lfvio_ctx lfvio_ctx;

/* Create a context on HIP device `device`.  Fails (returns NULL) when no
 * gfx950 device / HIP runtime is usable: there is no CPU fallback. */
lfvio_ctx *lfvio_create(int device);
void lfvio_destroy(lfvio_ctx *ctx);
const char *lfvio_last_error(const lfvio_ctx *ctx);
const char *lfvio_version(void);

/* ceres::Solve replacement for the problem built at estimator.cpp:678-825:
 * upload, run the trust-region loop on the device, download. */
int lfvio_solve(lfvio_ctx *ctx, const LfvioWindow *in, LfvioSolution *out);

/* MarginalizationInfo::{preMarginalize,marginalize,getParameterBlocks}
 * replacement for the factor sets built at estimator.cpp:833-1005.  `in` holds
 * the state AFTER double2vector()+vector2double().  For MARGIN_SECOND_NEW with
 * no prior touching Pose[WINDOW_SIZE-1] the reference does nothing
 * (estimator.cpp:942-943): out->valid is copied from the input prior. */
int lfvio_marginalize(lfvio_ctx *ctx, const LfvioWindow *in, int flag, LfvioPrior *out);

/* ---- relocalization: the loop-closure branch of optimization() (estimator.cpp:777-808) ------------------------------
 * A /pose_graph/match_points message stored by Estimator::setReloFrame (estimator.cpp:1133-1151) adds one parameter block,
 * relo_Pose (7 global / 6 local, PoseLocalParameterization, never constant, never part of the prior or of the
 * marginalization), and per matched landmark one PLAIN ProjectionFactor (factor/projection_factor.cpp: no td column even
 * with ESTIMATE_TD, same sqrt_info and CauchyLoss(1.0)) on (para_Pose[start_frame], relo_Pose, para_Ex_Pose, para_Feature[l])
 * with pts_i = the landmark's first observation and pts_j = (x, y, 1).  The host builds the match list by the reference's walk
 * (estimator.cpp:782-806): landmarks of the window's list (the LfvioWindow order) with start_frame <= frame, ids matched in
 * ascending order against match_points. */
typedef struct LfvioRelo {
  int frame;                         /* relo_frame_local_index, 0 .. LFVIO_WINDOW_SIZE - 1                        */
  double relo_pose[LFVIO_SIZE_POSE]; /* initial relo_Pose [p, q xyzw], as setReloFrame copied it from para_Pose  */
  int num_matches;                   /* K relocalization factors                                                  */
  const int *landmark;               /* [K] strictly ascending indices into the window's landmark list, each with
                                        start_frame[l] <= frame                                                     */
  const double *match_point;         /* [K][2] x, y of match_points: pts_j = (x, y, 1)                             */
} LfvioRelo;
/* lfvio_solve with the relocalization factors: the same conventions — outputs are the state before double2vector() (whose
 * relo tail, estimator.cpp:603-625, stays on the host) plus the solved relo pose; on error nothing is written; the trace
 * fields and max_solver_time_in_seconds are those of lfvio_solve.  LFVIO_ERR_ARG for a malformed relo (frame out of range,
 * num_matches < 0, NULL arrays with num_matches > 0, an index out of range, not strictly ascending, or of a landmark with
 * start_frame > frame) and for windows of more than 2048 landmarks on the relo route.  num_matches == 0 is the plain solve
 * with relo_pose copied through (Ceres drops a parameter block no residual uses).  The route is one launch sequence per
 * trust-region pass and one host synchronisation per pass: a relo solve happens once per loop-closure message. */
int lfvio_solve_relo(lfvio_ctx *ctx, const LfvioWindow *in, const LfvioRelo *relo, LfvioSolution *out,
                     double relo_pose_out[LFVIO_SIZE_POSE]);

/* ---- device-resident API (throughput / bench; same kernels) -------------
 * upload once, then run the whole optimization() — solve, the gauge fix of
 * double2vector() (estimator.cpp:532-600) and marginalization — without
 * leaving the device.  `batch` independent windows can be resident at once
 * (BASELINE config "512 independent windows"). */
int lfvio_batch_reserve(lfvio_ctx *ctx, int batch, int max_landmarks, int max_observations);
int lfvio_batch_upload(lfvio_ctx *ctx, int slot, const LfvioWindow *in);
/* run optimization() for slots [0, count): flag per call (same for all slots) */
int lfvio_batch_optimize(lfvio_ctx *ctx, int count, int marg_flag);
/* enqueue only (no host sync); stream is the context's stream */
int lfvio_batch_optimize_async(lfvio_ctx *ctx, int count, int marg_flag);
int lfvio_batch_sync(lfvio_ctx *ctx);
/* state returned here is AFTER the gauge fix (what Ps/Rs/Vs... hold after
 * double2vector()), re-expressed through vector2double(). */
int lfvio_batch_download(lfvio_ctx *ctx, int slot, LfvioSolution *sol, LfvioPrior *prior);
/* The same call split in two for ONE resident window (slot 0), for callers that use the state before they need the
 * prior — the reference publishes the pose right after optimization() (estimator_node.cpp:  pubOdometry behind
 * processImage) and reads last_marginalization_info first in the NEXT optimization() (estimator.cpp:700-706):
 *   lfvio_batch_optimize_begin   returns with the solution (after the gauge fix, as lfvio_batch_download gives it) as soon as
 *                                solve + gauge fix are out; the marginalization is still running on the device then
 *                                (lfvio_batch_optimize_pending() == 1).  The device pushes the state into mapped host memory and
 *                                the call polls one word of it: no copy, no stream synchronization in front of the caller.
 *   lfvio_batch_optimize_finish  waits for the rest and delivers the prior (NULL: just wait).  Any other entry point on the
 *                                context waits for the tail first, so forgetting it costs overlap, not correctness; the prior
 *                                must be collected before the slot is uploaded again.
 * lfvio_triangulate / lfvio_shift_depth / lfvio_preintegrate do NOT wait: they run beside the tail on their own stream. */
/* lfvio_batch_upload_chained  the upload of the NEXT window of the same estimator while that marginalization is still
 *                                running: the window's prior is *prior_io (in->prior is ignored), and if a call is in flight
 *                                on the context it is THAT call's prior — the landmark tables of the new window are packed
 *                                on the host while the device finishes, then the prior is collected into *prior_io (as
 *                                lfvio_batch_optimize_finish would) and goes up with the window.  With nothing in flight it
 *                                is lfvio_batch_upload with in->prior = prior_io. */
int lfvio_batch_upload_chained(lfvio_ctx *ctx, int slot, const LfvioWindow *in, LfvioPrior *prior_io);
/* lfvio_batch_upload_chained_device  the same hand-over WITHOUT the host in it (round 5): while the call begun with
 *                                lfvio_batch_optimize_begin is still marginalizing, the next window of the same estimator is
 *                                packed, its copies are enqueued behind that marginalization, and the prior it is producing becomes
 *                                this window's prior where it lies on the device (in->prior is ignored; the block structure is the one
 *                                this library planned for that marginalization, the values never leave the GPU).  Nothing is waited
 *                                for: the call returns as soon as the copies are enqueued, and the lfvio_batch_optimize_begin that
 *                                follows goes out behind them — the device runs window after window back to back, the caller still
 *                                gets every state as early as before (estimator.cpp:700-706: the prior is read by the NEXT
 *                                optimization(), which is exactly where it stays).  The prior of the call that was in flight is no
 *                                longer collectable afterwards (lfvio_batch_optimize_finish delivers the NEWEST call's prior).
 *                                LFVIO_ERR_ARG (nothing enqueued, the call in flight untouched) when there is no call in flight on
 *                                slot 0 or when its marginalization passes the input prior through (MARGIN_SECOND_NEW without a prior
 *                                on the newest pose): use lfvio_batch_upload_chained then.  If that marginalization fails on the
 *                                device — or leaves a prior of another block structure than the one promised — the window runs
 *                                without a prior and the next lfvio_batch_optimize_begin / lfvio_batch_optimize(ctx, 1, flag)
 *                                returns LFVIO_ERR_DEVICE.  Those two are the calls that may follow this upload: any other way
 *                                of optimizing the slot (lfvio_batch_optimize_async, a count above one) is refused with
 *                                LFVIO_ERR_ARG — the verdict on the prior travels with the graph of one window's synchronous call. */
int lfvio_batch_upload_chained_device(lfvio_ctx *ctx, int slot, const LfvioWindow *in);
int lfvio_batch_optimize_begin(lfvio_ctx *ctx, int marg_flag, LfvioSolution *sol);
int lfvio_batch_optimize_finish(lfvio_ctx *ctx, LfvioPrior *prior);
int lfvio_batch_optimize_pending(const lfvio_ctx *ctx);
/* the context's HIP stream (hipStream_t) for event timing by the caller */
void *lfvio_stream(lfvio_ctx *ctx);

/* ---- the landmark-parallel steps either side of optimization() ------------------------
 * lfvio_triangulate: FeatureManager::triangulate (feature_manager.cpp:199-253).  For every landmark with
 * estimated_depth <= 0 (the caller lists only landmarks with used_num >= 2 && start_frame < WINDOW_SIZE - 2, in the
 * CSR form of LfvioWindow): the 2k x 4 system of the k observations in the frame of the first one, its right singular
 * vector of the smallest singular value v (the reference: Eigen::JacobiSVD, ComputeThinV, last column),
 * depth = (v[0:3] / v[3]) . point_0, replaced by init_depth when negative.  Landmarks with estimated_depth > 0 are
 * left alone.  estimated_depth is read and written in place. */
typedef struct {
  int num_landmarks, num_observations;
  const int *start_frame;   /* [N] */
  const int *obs_offset;    /* [N + 1] */
  const double *obs_point;  /* [M][3]  FeaturePerFrame::point as stored (normalized inside, used raw in the dot product) */
  double Ps[LFVIO_NUM_FRAMES][3];
  double Rs[LFVIO_NUM_FRAMES][9]; /* row-major */
  double tic[3], ric[9];
  double init_depth;              /* INIT_DEPTH, parameters.cpp:116 */
} LfvioTriangulateIn;
int lfvio_triangulate(lfvio_ctx *ctx, const LfvioTriangulateIn *in, double *estimated_depth);

/* lfvio_shift_depth: the arithmetic of FeatureManager::removeBackShiftDepth (feature_manager.cpp:271-310) for the n
 * landmarks that started in the marginalized frame and keep >= 2 observations: uv_i is the erased first observation,
 * depth <- || new_R^T (marg_R (uv_i * depth) + marg_P - new_P) ||, or init_depth when that is not > 0.
 * (Erasing observations / features and start_frame-- stay list bookkeeping on the host.) */
int lfvio_shift_depth(lfvio_ctx *ctx, int n, const double *uv_i /* [n][3] */, const double marg_R[9], const double marg_P[3],
                      const double new_R[9], const double new_P[3], double init_depth, double *estimated_depth /* [n] */);

/* lfvio_preintegrate: IntegrationBase::push_back / propagate / midPointIntegration (factor/integration_base.h:29-158) for
 * num_intervals independent keyframe intervals at once — the ten of a window after a bias update (repropagate(),
 * integration_base.h:41-52, called from Estimator::double2vector / solveGyroscopeBias), or one interval as frames arrive.
 * Each interval is the constructor arguments (acc_0, gyr_0, linearized_ba, linearized_bg, integration_base.h:15-27) plus its
 * buffered samples dt_buf / acc_buf / gyr_buf; noise = {ACC_N, GYR_N, ACC_W, GYR_W} (parameters.cpp:94-97).  out[k] is
 * what LfvioWindow::imu[k] takes: delta_p/q/v, sum_dt, jacobian and covariance after the last sample.  An interval with
 * no samples returns the constructor state (identity jacobian, zero covariance). */
typedef struct {
  int num_samples;
  const double *dt;  /* [num_samples]    */
  const double *acc; /* [num_samples][3] */
  const double *gyr; /* [num_samples][3] */
  double acc_0[3], gyr_0[3], linearized_ba[3], linearized_bg[3];
} LfvioImuInterval;
int lfvio_preintegrate(lfvio_ctx *ctx, int num_intervals, const LfvioImuInterval *in, const double noise[4], LfvioPreintegration *out);

/* lfvio_two_view: the two-view step of ESTIMATE_EXTRINSIC == 2 — InitialEXRotation::solveRelativeR for >= 9 matches
 * (initial/initial_ex_rotation.cpp:157-284; cv::findFundamentalMat and the prints of :226-264 have no effect there and are
 * not restated).  An 8-point RANSAC on BEARING vectors (rays with z <= 0 are ordinary inputs): per sample set the null
 * vector of the 8 x 9 epipolar system, projected to rank 2 (compute_E_21, :69-100), scored by check_inliers (:101-155: the
 * float threshold 0.00872653549837f, a float score taking its double terms in match order); the first hypothesis with the
 * largest score > 0 wins (:197-202); compute_E_21 again over its inliers and check_inliers again (:204-218: that mask is
 * the one returned); decomposeE (:321-336) to R1 = U W V^T, R2 = U W^T V^T, t = +-u_2 (proper rotations: the reference
 * negates E and decomposes again when det R1 = -1, here u_2 and v_2 are the cross products of the other two columns —
 * the same four candidates; which of the two rotations is called R1 depends on the signs an SVD gives its vectors and is
 * not pinned); testTriangulation (:289-319, :338-353) of the four candidates in bearing form, IEEE semantics kept (a
 * null vector with a zero fourth entry gives inf / NaN and the match does not count); R_rel is the return value of
 * solveRelativeR: ratio1 > ratio2 ? R1 : R2, transposed (:276-284).
 * The sample sets are an INPUT (the reference draws them from std::random_device, util::create_random_array(8, 0, N - 1)),
 * which makes the call a function of its arguments.
 * Deviations from the reference: where no hypothesis scores above 0 the reference reads an uninitialised matrix and
 * throws from vector::at; where the winner has fewer than 8 inliers its refit is under-determined.  Both return
 * status = 1 here (best_sample = -1 and num_inliers = 0 in the first case, the winner and its count in the second), and
 * E, R_cand, t_cand, front, R_rel and the mask are left as the caller had them.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_matches outside [8, 4096], num_samples outside [1, 1024], a sample
 * index outside [0, num_matches).  Runs on the feature stream like lfvio_triangulate: it does not wait for an
 * optimization in flight. */
typedef struct {
  int num_matches;            /* N, 8 <= N <= 4096 */
  const double *bearing_l;    /* [N][3] FeaturePerFrame::point of the older frame, as stored (not renormalised) */
  const double *bearing_r;    /* [N][3] ... of the newer frame */
  int num_samples;            /* S hypotheses, 1 <= S <= 1024; the reference: 100 */
  const int *samples;         /* [S][8] indices into the matches */
} LfvioTwoViewIn;
typedef struct {
  int status;                 /* 0 model found; 1 no hypothesis scored > 0 or fewer than 8 inliers */
  int best_sample;            /* index of the winning hypothesis (first one wins a tie) */
  int num_inliers;
  double best_score;          /* of the winning hypothesis, before the refit */
  double E[9];                /* best_E_21 after the refit on its inliers, row-major, sign free */
  double R_cand[2][9], t_cand[3]; /* R1, R2 (both proper rotations), t = u_2; the four candidates are (R1|R2, +-t) */
  double front[4];            /* testTriangulation of (R1,t) (R1,-t) (R2,t) (R2,-t): front_count / N */
  double R_rel[9];            /* solveRelativeR()'s return value (the chosen candidate, transposed) */
} LfvioTwoViewOut;
int lfvio_two_view(lfvio_ctx *ctx, const LfvioTwoViewIn *in, unsigned char *inlier /* [N], after the refit */,
                   LfvioTwoViewOut *out, double *E_all /* [S][9] or NULL */, float *score_all /* [S] or NULL */);

/* lfvio_vi_align: the visual-inertial alignment of Estimator::initialStructure — VisualIMUAlignment
 * (initial/initial_aligment.cpp:3-216), literally as written, on poses of every image of the window that are known up to
 * scale in the camera frame of one keyframe (what relativePose / GlobalSFM::construct / the PnP loop leave in
 * all_image_frame, estimator.cpp:250-357).  The rest of Estimator::visualInitialAlign (:380-437) is the caller's.
 *   solveGyroscopeBias (:3-36): over the F - 1 consecutive pairs q_ij = Quaterniond(R_i^T R_j) (Eigen's matrix-to-quaternion
 *     branches), tmp_A = jacobian(O_R, O_BG), tmp_b = 2 (delta_q^-1 (x) q_ij).vec(), the 3 x 3 normal equations summed in pair
 *     order; then EVERY span is integrated again with ba = 0 and bg = Bgs[0] + delta_bg (:34), where Bgs[0] is
 *     span[1].linearized_bg as passed (the spans' own linearized_ba / linearized_bg are used by the first integration only).
 *   LinearAlignment (:121-206): the 6 x 10 blocks, n = 3F + 4, the / 100 on the scale column, x 1000 on A and b, both gates.
 *   RefineGravity (:53-119): TangentBasis with its exact `a == tmp` comparison, four iterations, n = 3F + 3.  A and b are zeroed
 *     ONCE, before the loop (:61-64), and scaled by 1000 inside it (:111-112): iteration k solves the sum of all blocks so far,
 *     each earlier set weighted 1000 x more than the next.  Kept as written; g_iter shows it.
 * Deviation from the reference: Eigen's ldlt() pivots and tolerates a semidefinite matrix; the device factors the arrowhead
 * (block-tridiagonal velocity part, dense border) without pivoting and returns status = 3 with every output but `status`
 * untouched when a pivot is not > 0 (e.g. all T equal: the scale column is zero).  With status 1 or 2 the fields computed before
 * the gate are written (delta_bg, g_linear, s_linear; with 2 also g_iter, g, s — the reference has moved Bgs by then); x and
 * pre are left as the caller had them.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_frames outside [4, LFVIO_MAX_IMAGE_FRAMES], a span k >= 1 with no
 * samples or sum_dt == 0.  F >= 4 because below it the systems are singular by counting: 6 (F - 1) equations against 3F + 4
 * unknowns (the reference only calls this with the full window, F >= 11).
 * One upload, one download and four launches in between (k_preintegrate twice, unchanged); runs on the feature stream like
 * lfvio_triangulate: it does not wait for an optimization in flight. */
#define LFVIO_MAX_IMAGE_FRAMES 128
typedef struct {
  int num_frames;               /* F in [4, LFVIO_MAX_IMAGE_FRAMES]: all_image_frame in stamp order */
  const double *R;              /* [F][9] ImageFrame::R, row-major (body rotation in the SfM frame, estimator.cpp:299,355) */
  const double *T;              /* [F][3] ImageFrame::T (camera position in the SfM frame, unscaled, :300,356) */
  const LfvioImuInterval *span; /* [F]    span[k]: the samples between image k - 1 and image k, constructor arguments as
                                          ImageFrame::pre_integration had them; span[0] is not read */
  double noise[4], tic[3], g_norm; /* ACC_N, GYR_N, ACC_W, GYR_W; TIC[0]; G.norm() */
} LfvioViAlignIn;
typedef struct {
  int status;                   /* 0 aligned; 1 first gate of LinearAlignment (initial_aligment.cpp:186);
                                   2 s < 0 after RefineGravity (:201); 3 a pivot that is not > 0 (deviation, above) */
  double delta_bg[3];           /* solveGyroscopeBias (:25) */
  double g_linear[3], s_linear; /* LinearAlignment before the refinement (:179-181) */
  double g_iter[4][3];          /* g0 after each of RefineGravity's four iterations (:115) */
  double g[3], s;               /* :118, :197 */
} LfvioViAlignOut;
int lfvio_vi_align(lfvio_ctx *ctx, const LfvioViAlignIn *in, LfvioViAlignOut *out,
                   double *x /* [3F] velocities of the last solve, body frames */,
                   LfvioPreintegration *pre /* [F] after the re-propagation, pre[0] untouched; or NULL */);

/* lfvio_pnp: PnpSolver::compute_pose (vins_estimator/src/pnp_solver.cpp) for num_frames frames at once — the EPnP on BEARING
 * vectors that poses every non-keyframe in the PnP loop of Estimator::initialStructure (estimator.cpp:288-357) and every keyframe
 * inside GlobalSFM::solveFrameByPnP (initial/initial_sfm.cpp:23-71).  Internal parameters are the reference's only call form,
 * set_internal_parameters(0, 0, 1, 1).  Frame f owns the correspondences offset[f] .. offset[f + 1] (a CSR): the SfM point and
 * FeaturePerFrame::point as stored (not renormalised; z <= 0 is an ordinary input).  Restated literally, quirks included:
 *   choose_control_points (:45-75): the mean, JacobiSVD of the 3 x 3 PW0^T PW0, k = sqrt(DC / n);
 *   compute_barycentric_coordinates (:76-96); M with its division by us(i, 2) (:313-325); M^T M and its four smallest singular
 *   vectors Ut(11 - i) (:326-333); compute_L_6x10 and compute_rho (:101-144);
 *   find_betas_0 / _1 / _2 (:145-230) over colPivHouseholderQr().solve with Eigen's rank threshold (a pivot column whose norm
 *     falls below eps x the largest column norm x sqrt((rows - k) / rows) ends the factorization; the dropped components are 0);
 *     `B5[0] = -B5[0]` of :226-227 comes after the last use of B5[0] and changes nothing — Betas[0] is NOT negated there;
 *   gauss_newton (:388-405): exactly 15 iterations, no convergence test;
 *   solve_for_sign (:246-254): the sign of the FIRST correspondence only;
 *   estimate_R_and_t (:255-284): R = U V^T with no determinant fix (a reflection is returned as such);
 *   reprojection_error (:285-296): the un-normalised camera point R p + T subtracted from the bearing, mean of squares;
 *   the winner (:355-369): strict <, the first candidate wins a tie.
 * R and T are what compute_pose returns (world to camera, before the caller's transpose of estimator.cpp:353-356).
 * After the 15 Gauss-Newton steps the three candidates usually agree to rounding, so `chosen` is decided by rounding: hold
 * R, T and err[chosen], not chosen.
 * Deviations from the reference:
 *   1. a non-finite value among err[0..2] or the winner's R, T (a bearing with z == 0; coplanar points, whose CC is singular)
 *      returns status = 1 for that frame and leaves R, T, err and chosen of that frame as the caller had them; the other frames
 *      of the call are not affected;
 *   2. the signs an SVD gives its vectors are not Eigen's.  For the null vectors of M^T M and the vectors of W the result does
 *      not depend on them beyond rounding.  For the principal axes of choose_control_points it does: flipping an axis moves a
 *      control point, and with noisy bearings the pose changes at the level of the noise (measured 1.4e-2 in R at 1 px,
 *      f = 160; below 2e-14 with exact bearings).  Here each axis gets the sign that makes its largest component (the first of
 *      equal ones) positive; which sign Eigen's JacobiSVD returns is not reproduced;
 *   3. M^T M is summed as the 40 distinct sums a_j a_k {1, x, y, x^2 + y^2}, x = (0 - u_0) / u_2, y = (0 - u_1) / u_2; these, W and
 *      the means are summed in the device's own fixed order (no atomics): a call returns the same bits every time and a
 *      batch of F frames returns the bits of F single-frame calls.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_frames outside [1, LFVIO_MAX_IMAGE_FRAMES], offset[0] != 0, a frame
 * with fewer than 6 or more than 4096 correspondences (which covers an offset array that is not ascending).
 * One upload, one launch (one workgroup per frame), one download; runs on the feature stream like lfvio_triangulate: it
 * does not wait for an optimization in flight. */
typedef struct {
  int num_frames;        /* F in [1, LFVIO_MAX_IMAGE_FRAMES] */
  const int *offset;     /* [F + 1] offset[0] = 0, 6 <= offset[f + 1] - offset[f] <= 4096 */
  const double *point_w; /* [M][3] SfM points, M = offset[F] */
  const double *bearing; /* [M][3] FeaturePerFrame::point of the frame, as stored */
} LfvioPnpIn;
typedef struct {
  int status;            /* 0 posed; 1 a non-finite value (deviation 1) */
  int chosen;            /* index of the winning candidate (decided by rounding, see above) */
  double R[9], T[3];     /* compute_pose's R (row-major) and T: x_cam = R x_w + T */
  double err[3];         /* reprojection_error of the candidates of find_betas_0 / _1 / _2 */
} LfvioPnpOut;
int lfvio_pnp(lfvio_ctx *ctx, const LfvioPnpIn *in, LfvioPnpOut *out /* [F] */);

/* lfvio_sfm_ba: the "full BA" that ends GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:233-309) — the second of the
 * reference's two ceres::Solve calls.  The incremental part of construct() (:121-218) is lfvio_sfm_construct below and relativePose()
 * is lfvio_relative_pose: their outputs are this call's inputs.
 *   :237-257  parameter blocks c_rotation[i] (4, w x y z, world to camera, QuaternionParameterization) and c_translation[i] (3);
 *             the rotation of frame l constant (:249-252), the translations of frames l and frame_num - 1 constant (:253-256);
 *   :259-275  one ReprojectionError3D (initial_sfm.h:25-63) per observation of every sfm_f entry with state == true, no loss:
 *             r = p / |p| - bearing, p = R(q / |q|) X + t (ceres::QuaternionRotatePoint normalises), the bearing as stored (not
 *             renormalised; z <= 0 is an ordinary input); the caller lists only those entries, in sfm_f order, as a CSR;
 *   :276-281  DENSE_SCHUR, every other option Ceres' default: TrustRegionMinimizer with the Levenberg-Marquardt strategy (initial
 *             radius 1e4; the diagonal sqrt(clamp(diag J^T J, 1e-6, 1e32) / radius) on every column; on success radius <- min(1e16,
 *             radius / max(1/3, 1 - (2 rho - 1)^3)), on rejection radius <- radius / factor, factor <- 2 factor), Jacobi scaling fixed
 *             at iteration 0, min_relative_decrease 1e-3, the three tolerance tests, five consecutive invalid steps -> LFVIO_FAILURE;
 *             DESIGN.md §3h lists every row of that policy and where it comes from — parity with Ceres itself is not pinned;
 *   :283      accepted = termination == LFVIO_CONVERGENCE || final_cost < 5e-3 (the caller returns false when it is 0);
 *   :295-309  Q[i] = the inverse of c_rotation[i] (conjugate / squared norm), T[i] = -(Q[i] * c_translation[i]).
 * c_rotation [F][4], c_translation [F][3] and position [P][3] (sfm_f[j].position of the listed entries) are read and, on LFVIO_OK,
 * written as Ceres leaves them (:240-246, :273); the constant blocks come back bit for bit.  x [+] delta = [cos|delta|, sin|delta| /
 * |delta| delta] (x) x with no renormalisation afterwards: a rotation keeps the norm it came with.  The trace holds iteration 0 too,
 * as LfvioSolution has it; the entry of a step that was not successful has gradient_max_norm 0.
 * Options: a tolerance <= 0 takes Ceres' default (1e-6, 1e-10, 1e-8); max_num_iterations < 0 takes 50, 0 is iteration 0 alone (the
 * evaluation at the start, as in Ceres), at most LFVIO_MAX_TRACE - 1.  The fields exist so that a test can force convergence.
 * Deviations from the reference:
 *   1. max_solver_time_in_seconds = 0.2 (:279) is NOT honoured: the loop runs on the device without a host round trip and ends on
 *      its tolerances or its iteration cap;
 *   2. a non-finite initial cost returns LFVIO_ERR_NONFINITE with every output untouched (Ceres would report FAILURE);
 *   3. every sum runs in the device's own fixed order (no atomics): a repeated call returns the same bits.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_frames outside [2, LFVIO_NUM_FRAMES], ref_frame outside [0, F - 2], num_points
 * outside [1, 4096], obs_offset[0] != 0, a point with no observation or more than F (which covers an offset array that is not
 * ascending), an obs_frame outside [0, F), a frame listed twice for one point, max_num_iterations > LFVIO_MAX_TRACE - 1.
 * A frame may have no observation at all: its blocks do not move.  One upload, one launch (one workgroup), one download; runs on the
 * feature stream like lfvio_pnp: it does not wait for an optimization in flight. */
typedef struct {
  int num_frames;            /* F = frame_num, in [2, LFVIO_NUM_FRAMES] */
  int ref_frame;             /* l, in [0, F - 2] */
  int num_points;            /* P in [1, 4096] */
  const int *obs_offset;     /* [P + 1] obs_offset[0] = 0, 1 <= obs_offset[j + 1] - obs_offset[j] <= F */
  const int *obs_frame;      /* [M] observation.first, M = obs_offset[P] */
  const double *obs_bearing; /* [M][3] observation.second, as stored */
  int max_num_iterations;    /* < 0: 50 */
  double function_tolerance, gradient_tolerance, parameter_tolerance; /* <= 0: 1e-6, 1e-10, 1e-8 */
} LfvioSfmBaIn;
typedef struct {
  int termination;           /* LFVIO_CONVERGENCE / LFVIO_NO_CONVERGENCE / LFVIO_FAILURE */
  int num_iterations;        /* iteration 0 included */
  int num_successful_steps, num_unsuccessful_steps;
  int accepted;              /* :283 */
  int pad_;
  double initial_cost, final_cost; /* 1/2 sum r^2, as summary.final_cost */
  double Q[LFVIO_NUM_FRAMES][4];   /* w x y z; rows >= F untouched */
  double T[LFVIO_NUM_FRAMES][3];
  LfvioIterationSummary trace[LFVIO_MAX_TRACE];
} LfvioSfmBaOut;
int lfvio_sfm_ba(lfvio_ctx *ctx, const LfvioSfmBaIn *in, double *c_rotation /* [F][4] */, double *c_translation /* [F][3] */,
                 double *position /* [P][3] */, LfvioSfmBaOut *out);

/* lfvio_sfm_construct: the incremental part of GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:121-218) — from the
 * relative pose of frames l and frame_num - 1 (what relativePose() returns: lfvio_relative_pose below) to a pose per keyframe and a
 * position per point, which are lfvio_sfm_ba's in/out arrays.  The schedule, literally; an "op" is one step of it, numbered from 0:
 *   :125-153  q[l] = 1, T[l] = 0, q[F - 1] = q[l] * Quaterniond(relative_R), T[F - 1] = relative_T; for both, c_Quat = q.inverse()
 *             (conjugate / squared norm), c_Rotation = c_Quat.toRotationMatrix(), c_Translation = -1 * (c_Rotation * T).  Eigen's
 *             matrix to quaternion conversion with its four branches (trace > 0, else the largest diagonal entry);
 *   :157-175  for i = l .. F - 2: if i > l, solveFrameByPnP(i) [one op]; triangulateTwoFrames(i, F - 1) [one op];
 *   :177-178  for i = l + 1 .. F - 2: triangulateTwoFrames(l, i) [one op each];
 *   :181-195  for i = l - 1 .. 0: solveFrameByPnP(i) [one op]; triangulateTwoFrames(i, l) [one op];
 *   :197-218  the closing loop [ONE op]: every point still untriangulated with >= 2 observations, from its first and last one.
 * 3 F - 4 - l ops in all.  solveFrameByPnP (:23-71) takes the points with state == true that have an observation in frame i, in
 * ascending j, and is lfvio_pnp's compute_pose on them (same kernel code, same bits); fewer than 10 returns false (:51-52).  Its
 * result is the frame's c_Rotation, c_Translation; c_Quat[i] = c_Rotation[i] (:168, :190) is the same matrix to quaternion
 * conversion, applied even when compute_pose returned a reflection.  triangulateTwoFrames (:73-110) takes every point with
 * state == false seen in both frames; triangulatePoint (:6-21) takes the right singular vector of the smallest singular value of the
 * 4 x 4 design matrix and divides by its fourth entry, with IEEE semantics: a zero fourth entry gives inf / NaN in that position and
 * the chain goes on.  A position is written once and never changes.
 * Outputs: c_rotation[i] = c_Quat[i] (w x y z), c_translation[i] = c_Translation[i] as :240-246 hand them to Ceres; position[j]
 * (0, 0, 0 for a point that stays untriangulated); tri_op[j] = the op that set state = true for point j, or -1.  position compacted
 * to the points with tri_op >= 0, with their observations, is what :259-275 hand to Ceres: with c_rotation and c_translation these
 * are exactly lfvio_sfm_ba's arrays.
 * Deviations from the reference:
 *   1. where the finiteness gate of the PnP trips (lfvio_pnp, deviation 1) the chain stops with status 2; the reference would carry
 *      the NaN on.  out->pnp[f] of that frame holds status 1 and the non-finite record as computed;
 *   2. on status 1 or 2 the outputs hold what the chain had when it stopped: rows of c_rotation, c_translation of frames not yet
 *      posed are left as the caller had them, position and tri_op are written for every point (the reference returns false and its
 *      caller drops everything);
 *   3. a frame listed twice for one point is LFVIO_ERR_ARG, as in lfvio_sfm_ba (the two scans of the reference, :34-46 and :87-99,
 *      disagree on which of two duplicates they take);
 *   4. the signs an SVD gives its vectors are lfvio_pnp's (its deviation 2: the principal axes pinned by this project's rule); a
 *      triangulated point does not depend on the sign of its singular vector;
 *   5. every sum runs in the device's own fixed order (no atomics): a repeated call returns the same bits.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_frames outside [2, LFVIO_NUM_FRAMES], ref_frame outside [0, F - 2], num_points
 * outside [1, 4096], obs_offset[0] != 0, a point with no observation or more than F (which covers an offset array that is not
 * ascending), an obs_frame outside [0, F), a frame listed twice for one point.
 * One upload, one launch (one workgroup), one download; runs on the feature stream like lfvio_sfm_ba: it does not wait for an
 * optimization in flight. */
typedef struct {
  int num_frames;            /* F = frame_num, in [2, LFVIO_NUM_FRAMES] */
  int ref_frame;             /* l, in [0, F - 2] */
  int num_points;            /* P in [1, 4096]: ALL of sfm_f, in sfm_f order */
  const int *obs_offset;     /* [P + 1] obs_offset[0] = 0, 1 <= obs_offset[j + 1] - obs_offset[j] <= F */
  const int *obs_frame;      /* [M] observation.first, M = obs_offset[P] */
  const double *obs_bearing; /* [M][3] observation.second, as stored */
  double relative_R[9];      /* row-major */
  double relative_T[3];
} LfvioSfmConstructIn;
typedef struct {
  int status;        /* 0 chain complete; 1 solveFrameByPnP returned false (< 10 correspondences, :51-52); 2 a PnP with a non-finite result */
  int failed_frame;  /* the frame of status 1 / 2, else -1 */
  int num_triangulated;
  int pad_;
  int pnp_op[LFVIO_NUM_FRAMES];    /* op index of the frame's PnP, -1 for l, F - 1 and frames not reached */
  int pnp_count[LFVIO_NUM_FRAMES]; /* correspondences it was given (0 where pnp_op is -1) */
  LfvioPnpOut pnp[LFVIO_NUM_FRAMES]; /* compute_pose's record of the frame (zeros where pnp_op is -1 or the count was below 10) */
} LfvioSfmConstructOut;
int lfvio_sfm_construct(lfvio_ctx *ctx, const LfvioSfmConstructIn *in, double *c_rotation /* [F][4] w x y z */,
                        double *c_translation /* [F][3] */, double *position /* [P][3] */, int *tri_op /* [P] */,
                        LfvioSfmConstructOut *out);

/* lfvio_relative_pose: Estimator::relativePose (vins_estimator/src/estimator.cpp:445-473) — the candidate loop over the pairs
 * (frame p, newest frame), p = 0 .. P - 1, with MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:536-576) behind it, ALL
 * pairs in one call.  Its l, relative_R, relative_T are lfvio_sfm_construct's inputs: with this call initialStructure() takes
 * nothing from outside.  Pair p owns the matches match_offset[p] .. match_offset[p + 1] (a CSR): getCorresponding(p, WINDOW_SIZE),
 * FeaturePerFrame::point as stored (not renormalised; z < 0 is an ordinary input).  Per pair, literally where the reference is
 * defined:
 *   :452      N <= 20: the pair is skipped (gate 1; this implies the >= 15 of solve_5pts.cpp:538);
 *   :454-463  average_parallax: per match |(x_l/z_l, y_l/z_l) - (x_r/z_r, y_r/z_r)| in double, summed in match order into one
 *             double, divided by N.  IEEE semantics kept: a ray with z == 0 gives inf or NaN;
 *   :464      !(average_parallax * 160 > 30): the pair is skipped (gate 2; 160, not 460: this tree's value; NaN > 30 is false);
 *   solve_5pts.cpp:275-335  myfindFundamentalMat: the 8-point RANSAC on bearings, the refit over the winner's inliers and its mask.
 *             compute_E_21 (:201-230) and check_inliers (:231-273) are those of initial_ex_rotation.cpp: this is lfvio_two_view's
 *             arithmetic, bit for bit on the same matches and sample sets (best_sample, best_score, num_inliers, the mask, E,
 *             R_cand, t_cand).  The threshold 0.3 / 460, the confidence and cv::findFundamentalMat of :554-558 have no effect and
 *             are not restated.  The sample sets are an INPUT, as for lfvio_two_view, local to the pair;
 *   :395-535  recoverPose over ALL N matches (_mask is not a filter here, unlike OpenCV's): for each of (R1,t) (R2,t) (R1,-t)
 *             (R2,-t) the point is triangulatePoint's 4 x 4 null vector divided by its fourth entry (:364-379), and it counts
 *             when b_l . Q / |Q| > 0 && b_r . Q' / |Q'| > 0 (:436-440; the divisions by the norms are kept, so a non-finite
 *             point does not count); the choice is the >= chain of :507-534, in that order.  Which rotation is called R1
 *             follows the signs an SVD gives its vectors and is not pinned (lfvio_two_view);
 *   :570      ok = inlier_cnt > 12.
 * l is the first pair with gate == 0 && ok; relative_R / relative_T are that pair's rotation / translation.
 * Deviations from the reference:
 *   1. the OUTPUT.  As shipped, recoverPose takes _R, _t and _mask BY VALUE (:395-396) and solveRelativeRT forms Rotation and
 *      Translation from uninitialised locals R, T (:566-569): there is no behaviour to restate.  The intent is unambiguous and is
 *      what is returned: rotation = rot^T, translation = -rot^T trans with (rot, trans) the candidate recoverPose chose — the
 *      rotation and unit-norm position of the newest camera in the frame of camera p, which is what lfvio_sfm_construct takes;
 *   2. where no hypothesis scores above 0, or the winner has fewer than 8 inliers, the reference reads an uninitialised matrix
 *      or refits an under-determined system (lfvio_two_view's status 1): the pair gets gate 3, with best_sample, num_inliers and
 *      best_score as lfvio_two_view reports them, and is passed over;
 *   3. ALL pairs are evaluated and reported, not only those up to l (the reference stops at the first success).  That changes
 *      nothing in l, relative_R, relative_T;
 *   4. every sum runs in a fixed order (the integer counts alone are added atomically): a repeated call returns the same bits.
 * A pair that did not run (gate 1 or 2) has best_sample = chosen = -1 and zeros in the fields behind average_parallax; a pair with
 * gate 3 has chosen = -1 and zeros behind best_score.  inlier (when not NULL) receives the refit mask of every pair with gate 0;
 * the slices of the other pairs stay as the caller had them.
 * LFVIO_ERR_ARG (outputs untouched): null pointers, num_pairs outside [1, LFVIO_WINDOW_SIZE], num_samples outside [1, 1024],
 * match_offset[0] != 0, a descending offset, a pair with more than 4096 matches, a sample index outside [0, N_p) for a pair with
 * N_p > 20 (the sample slots of a pair with N_p <= 20 are never read).
 * One upload, two launches (k_rp_hyp: a wave per (hypothesis, pair) and one per pair's parallax; k_rp_fit: a workgroup per pair),
 * one download; runs on the feature stream like lfvio_two_view: it does not wait for an optimization in flight. */
typedef struct {
  int num_pairs;             /* P in [1, LFVIO_WINDOW_SIZE]: pair p = getCorresponding(p, WINDOW_SIZE), in the reference's order */
  const int *match_offset;   /* [P + 1] CSR over the pairs' matches, match_offset[0] = 0, 0 <= N_p <= 4096 */
  const double *bearing_l;   /* [M][3] FeaturePerFrame::point of frame p, as stored */
  const double *bearing_r;   /* [M][3] ... of the newest frame */
  int num_samples;           /* S in [1, 1024]; the reference: 100 */
  const int *samples;        /* [P][S][8] indices LOCAL to the pair; read (and validated) only for pairs with N_p > 20 */
} LfvioRelativePoseIn;
typedef struct {
  int gate;                  /* 0 ran; 1 N <= 20 (:452); 2 !(average_parallax * 160 > 30) (:464); 3 no model (lfvio_two_view's status 1) */
  int num_matches, best_sample, num_inliers;   /* as LfvioTwoViewOut; num_inliers after the refit */
  double average_parallax;   /* :454-463, unscaled */
  double best_score;
  double E[9], R_cand[2][9], t_cand[3];        /* as LfvioTwoViewOut */
  int good[4];               /* recoverPose's good1..good4: (R1,t) (R2,t) (R1,-t) (R2,-t) — NOT front[]'s order */
  int chosen, inlier_cnt;    /* :507-534 with its >= chain; inlier_cnt = good[chosen] */
  int ok, pad_;              /* inlier_cnt > 12 (:570) */
  double rot[9], trans[3];   /* the chosen candidate */
  double rotation[9], translation[3];          /* rot^T, -rot^T trans (deviation 1) */
} LfvioRelativePosePair;
typedef struct {
  int l;                     /* first p with gate == 0 && ok, else -1 (relativePose() returned false) */
  int pad_;
  double relative_R[9], relative_T[3];         /* pair l's rotation / translation; untouched when l == -1 */
  LfvioRelativePosePair pair[LFVIO_WINDOW_SIZE]; /* entries >= P untouched */
} LfvioRelativePoseOut;
int lfvio_relative_pose(lfvio_ctx *ctx, const LfvioRelativePoseIn *in, unsigned char *inlier /* [M] refit masks, or NULL */,
                        LfvioRelativePoseOut *out);

/* lfvio_klt_track: the optical flow of FeatureTracker::readImage — cv::calcOpticalFlowPyrLK(cur_img, forw_img, cur_pts, forw_pts,
 * status, err, cv::Size(41, 41), 3) at feature_tracker/src/feature_tracker.cpp:127 and the inBorder test of :6-12, :129-131.  The
 * goodFeaturesToTrack and setMask are lfvio_gft_detect below, the CLAHE of :101-107 is lfvio_clahe_set below them, rejectWithF and
 * undistortedPoints are lfvio_track_reject / lfvio_track_undistort below those, and lfvio_track_frame below them runs all
 * of them, with reduceVector and updateID, on a track table resident in the context, and lfvio_track_frame_message adds the node's
 * feature message, and lfvio_track_batch_frame below that takes many independent image streams through it in one batched call; what
 * stays the caller's is the node's bookkeeping around that call — the first image dropped, the discontinuity
 * restart, the FREQ gate, the skipped first publication: host/image_gate.h and host/feature_tracker.h, on images in the trace format.
 * One call uploads `image`, builds its pyramid, tracks the N points from the pyramid of the PREVIOUS call's image (resident in the
 * context: cur_img = forw_img, :180) into the new one, and makes the new pyramid the resident one.  A context with no resident image —
 * after lfvio_create, after lfvio_klt_reset, or when width or height differ from the resident image's — treats `image` as both
 * images (:111-114).
 *   levels    level k + 1 is pyrDown of level k: separable [1 4 6 4 1] / 16, reflect-101 borders, even pixels, size ((w + 1) / 2,
 *             (h + 1) / 2), integer sums rounded (s + 128) >> 8.  Building stops before the first level whose width or height is
 *             <= win_size; levels_used is the last level built, capped by max_level.
 *   gradients Scharr 3 / 10 / 3 over 32 on the uint8 level, reflect-101 neighbours at the edge.  Outside a level the image continues
 *             by (repeated) reflect-101 and both gradients are 0.
 *   a point   for level L = levels_used .. 0: prev = p / 2^L; the guess is prev at the top level and twice the level above's result
 *             below it, and is the level's result until an iteration replaces it; the window's corner is prev - (win_size - 1) / 2
 *             with integer part ip; ip.x < -win_size, ip.x >= cols, ip.y < -win_size or ip.y >= rows skips the level (status 0 at
 *             level 0); A = sum g g^T / 1024 over the bilinear win x win patch, minEig = (A11 + A22 - sqrt((A11 - A22)^2 +
 *             4 A12^2)) / (2 win^2); minEig < min_eig_threshold or det A < FLT_EPSILON skips the level (status 0 at level 0);
 *             otherwise at most max_iterations times: the same bounds test on the guess's corner (failing it ends the level, status
 *             0 at level 0), b = sum (J - I) g / 1024, delta = ((A12 b2 - A22 b1) / det, (A12 b1 - A11 b2) / det), guess += delta;
 *             stop when delta . delta <= epsilon^2; from the second iteration on, when both components of |delta + previous delta|
 *             are < 0.01, take back delta / 2 and stop.
 *   after level 0: the border test; next_pts (rounded to float) is written for EVERY point, status 0 included.
 * tests/klt_ref.py restates this in numpy and is the specification.  Deviations from OpenCV: its fixed-point
 * interpolation (14-bit weights, 5 fractional bits in the patch) is plain floating point here; `err` is not produced — the tracker
 * never reads it.
 * LFVIO_ERR_ARG (every output and the resident image untouched): null ctx / in / image / next_pts / status / out, prev_pts null with
 * N > 0, or a field outside the range noted beside it.  Runs on the feature stream like lfvio_two_view: it does not wait for an
 * optimization in flight.  The pyramids live in device memory of their own, not in the feature calls' staging block. */
#define LFVIO_KLT_MAX_POINTS 4096
#define LFVIO_KLT_MAX_LEVEL 5
typedef struct {
  int width, height;           /* 8-bit grey image, rows contiguous (or as lfvio_image_format_set says); 16 <= width, height <= 8192 */
  const unsigned char *image;  /* forw_img */
  int num_points;              /* N, 0 <= N <= 4096: cur_pts */
  const float *prev_pts;       /* [N][2] x, y in the image of the PREVIOUS call (cv::Point2f) */
  int win_size;                /* odd, 5..41; the reference: 41 */
  int max_level;               /* 0..5; the reference: 3 */
  int max_iterations;          /* 1..100; OpenCV's default criteria: 30 */
  double epsilon;              /* > 0; default criteria: 0.01 (compared squared, as OpenCV does) */
  double min_eig_threshold;    /* >= 0; default 1e-4 */
  int border;                  /* inBorder() of :6-12 and :129-131: status 0 where the point, rounded half to even
                                  like cvRound, is outside [border, width-border) x [border, height-border);
                                  negative: no test; the reference: 1 */
} LfvioKltIn;
typedef struct { int levels_used; int num_tracked; } LfvioKltOut;
int lfvio_klt_track(lfvio_ctx *ctx, const LfvioKltIn *in, float *next_pts /* [N][2] */, unsigned char *status /* [N] */,
                    int *iterations /* [N][max_level+1], level 0 first, or NULL */, LfvioKltOut *out);
int lfvio_klt_reset(lfvio_ctx *ctx);   /* forget the resident image */
/* A level of the resident pyramid (0 .. the last level a call has built of it): its size and, where pixels is not NULL, its
 * width * height bytes.  LFVIO_ERR_ARG without a resident image or for a level that is not built. */
int lfvio_klt_level(lfvio_ctx *ctx, int level, int *width, int *height, unsigned char *pixels /* or NULL */);

/* lfvio_gft_detect: the other half of FeatureTracker::readImage — setMask() (feature_tracker/src/feature_tracker.cpp:46-83) and
 * cv::goodFeaturesToTrack(forw_img, n_pts, MAX_CNT - forw_pts.size(), 0.01, MIN_DIST, mask) (:147-176) on the image that
 * lfvio_klt_track left resident: level 0 of its pyramid (a call with N = 0 makes an image resident without tracking).  Tracked
 * points and counts go up, kept indices and new corners come down; the image does not move.
 *   response  Shi-Tomasi, block 3, Sobel 3: dx, dy = the 3 x 3 Sobel responses of the image continued by reflect-101; a, b, c = the
 *             3 x 3 box sums of dx^2, dx dy, dy^2, THESE maps continued by reflect-101 (not the gradients of the reflected image);
 *             S = a + c, D = (a - c)^2 + 4 b^2 as integers; lambda = 0.5 * (double(S) - sqrt(double(D))) >= 0.  OpenCV's value is
 *             lambda / (12 * 255)^2: only ratios are used, the factor is not applied.
 *   thinning  the points in order of descending track_cnt, equal counts by ascending index; (px, py) = the coordinates rounded half
 *             to even (cvRound); a point is dropped when a coordinate is NaN or the pixel is outside the image, when the base mask
 *             is not 255 there, or when an already kept point q has (px - qx)^2 + (py - qy)^2 <= mask_radius^2; otherwise it is
 *             kept.  The final mask is the base mask with zeros in every kept point's disc <= mask_radius^2.
 *   detection budget = max_count - num_kept; budget <= 0: no corners (num_candidates 0, max_response 0).  max_response = the
 *             largest lambda where the final mask is not 0, border rows included; 0 or no such pixel: no corners.  thr =
 *             quality_level * max_response.  A candidate: 1 <= x <= w - 2, 1 <= y <= h - 2, lambda > thr, lambda >= the lambda of
 *             each of its 8 neighbours (these NOT masked), final mask not 0.  Order: descending lambda, equal lambda by descending
 *             y * w + x.  Greedy: accepted when every accepted (x', y') has (x - x')^2 + (y - y')^2 >= min_distance^2; stops at
 *             `budget` accepted; corners are (float) x, (float) y in acceptance order.
 * tests/gft_ref.py restates this in numpy and is the specification; the device gives its bits.  Stated deviations
 * from the reference: equal counts are ordered by index (std::sort leaves them unspecified), discs are Euclidean (cv::circle differs
 * in a few rim pixels), a point outside the image is dropped (the reference reads out of bounds).
 * The base mask (fisheye_mask, or the annulus of :53-56) is device memory of the context: lfvio_gft_set_mask uploads it once, it
 * survives lfvio_klt_reset and every other call, and it is all 255 until set (pixels = NULL: all 255 again, width and height
 * ignored).  lfvio_gft_response gives lambda of the resident image, [height][width] doubles.
 * LFVIO_ERR_ARG (every output, the resident image and the base mask untouched): null ctx / in / corners / out / response, kept, pts
 * or track_cnt null with N > 0, a field outside the range noted beside it, no resident image, a base mask whose size is not the
 * resident image's (for lfvio_gft_set_mask: outside [16, 8192], or not the size of an image that is resident).  The calls run on
 * the feature stream like lfvio_klt_track: they do not wait for an optimization in flight. */
#define LFVIO_GFT_MAX_CORNERS 4096
typedef struct {
  int num_points;          /* N, 0 .. LFVIO_KLT_MAX_POINTS */
  const float *pts;        /* [N][2], forw_pts after the flow and rejectWithF; may be NULL when N = 0 */
  const int *track_cnt;    /* [N] */
  int max_count;           /* MAX_CNT, 1 .. LFVIO_GFT_MAX_CORNERS */
  double quality_level;    /* the reference: 0.01; in (0, 1] */
  int min_distance;        /* MIN_DIST for the new corners, 0 .. 1024 */
  int mask_radius;         /* MIN_DIST for the discs of setMask, 0 .. 1024 */
} LfvioGftIn;
typedef struct { int num_kept, num_corners, num_candidates; double max_response; } LfvioGftOut;
int lfvio_gft_detect(lfvio_ctx *ctx, const LfvioGftIn *in, int *kept /* [N] indices in kept order; num_kept written */,
                     float *corners /* [max_count][2]; num_corners written */, LfvioGftOut *out);
int lfvio_gft_set_mask(lfvio_ctx *ctx, int width, int height, const unsigned char *pixels /* NULL: all 255 */);
int lfvio_gft_response(lfvio_ctx *ctx, double *response /* [h][w] of the resident image */);

/* lfvio_clahe_set / lfvio_clahe_apply: the equalize step of FeatureTracker::readImage — cv::createCLAHE(3.0, cv::Size(8, 8))->
 * apply(_img, img) at feature_tracker/src/feature_tracker.cpp:101-107 (EQUALIZE = 1), on 8 bits.
 *   extent    width % tiles_x == 0 and height % tiles_y == 0: the image itself.  Otherwise the image continued right and down by
 *             (repeated) reflect-101 to (width + tiles_x - width % tiles_x) x (height + tiles_y - height % tiles_y): a side that does
 *             divide grows by a whole tiles_x (tiles_y), as in OpenCV.  tw, th = extent / tiles; area = tw th.
 *   clip      0 when clip_limit == 0, otherwise max((int)(clip_limit * area / 256), 1), in double.
 *   a tile    its 256-bin histogram in the extended image; with clip > 0: clipped = sum max(hist - clip, 0), hist = min(hist, clip),
 *             every bin += clipped / 256, and with rest = clipped % 256 != 0 and step = max(256 / rest, 1) the bins 0, step, 2 step,
 *             ... take one more each until `rest` are handed out.  lut[i] = saturate(round half even((float)(sum of hist[0 .. i]) *
 *             (255.0f / (float)area))).
 *   a pixel   (x, y) of the original width x height with value v: txf = (float)x * (1.0f / (float)tw) - 0.5f, tx1 = floor(txf),
 *             xa = txf - tx1, xa1 = 1.0f - xa, then tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0); the same in y; out =
 *             saturate(round half even((L[ty1][tx1][v] xa1 + L[ty1][tx2][v] xa) ya1 + (L[ty2][tx1][v] xa1 + L[ty2][tx2][v] xa) ya))
 *             in float, EVERY operation rounded on its own: a fused multiply-add gives other bytes.
 * tests/clahe_ref.py restates this in numpy and is the specification; the device gives its bits.
 * lfvio_clahe_set: cfg != NULL: every later lfvio_klt_track equalizes its image before the pyramid is built, so the resident image
 * is the equalized one (forw_img): lfvio_klt_level(ctx, 0, ...) returns it, the higher levels are pyrDown of it, lfvio_gft_detect and
 * lfvio_gft_response see it.  cfg == NULL: off, and lfvio_klt_track does what it does without this call.  Off after lfvio_create;
 * survives lfvio_klt_reset.
 * lfvio_clahe_apply: one image in, the equalized image out; lut (or NULL) receives [tiles_y][tiles_x][256] bytes.  Touches neither
 * the resident image nor the setting of lfvio_clahe_set.
 * LFVIO_ERR_ARG (every output, the resident image and the setting untouched): null ctx / pixels / out, null cfg in lfvio_clahe_apply,
 * a field outside its range, a NaN clip_limit, width or height outside [16, 8192].  Both run on the feature stream like
 * lfvio_klt_track: they do not wait for an optimization in flight. */
#define LFVIO_CLAHE_MAX_TILES 16
typedef struct {
  double clip_limit;    /* 0 .. 1024; the reference: 3.0; 0: no clipping */
  int tiles_x, tiles_y; /* 1 .. 16 each; the reference: 8, 8 */
} LfvioClaheIn;
int lfvio_clahe_set(lfvio_ctx *ctx, const LfvioClaheIn *cfg /* NULL: off */);
int lfvio_clahe_apply(lfvio_ctx *ctx, const LfvioClaheIn *cfg, int width, int height, const unsigned char *pixels,
                      unsigned char *out /* [height][width] */, unsigned char *lut /* [tiles_y][tiles_x][256], or NULL */);

/* lfvio_image_format_set / lfvio_image_gray: colour and 16-bit camera images — what cv_bridge::toCvCopy(img_msg, MONO8) does in
 * front of FeatureTracker::readImage (feature_tracker/src/feature_tracker_node.cpp:64-78) — converted on the device, in the write of
 * level 0 of the fresh pyramid.  One code space, the ABI's and the type-10 record's (host/replay.h):
 *
 *   code  name                              bytes / pixel  grey value
 *   0     LFVIO_IMG_MONO8 (also 8UC1)       1              v
 *   2     LFVIO_IMG_BGR8                    3              (1868 B + 9617 G + 4899 R + 8192) >> 14
 *   3     LFVIO_IMG_RGB8                    3              the same on R, G, B in their places
 *   4     LFVIO_IMG_BGRA8                   4              the same; the fourth byte is never read into the value
 *   5     LFVIO_IMG_RGBA8                   4              the same
 *   6     LFVIO_IMG_MONO16 (little endian)  2              (v + 128) / 257, integer division
 *   7     LFVIO_IMG_MONO16_BE               2              the same after the byte swap
 *
 * Code 1 and every code above 7 are refused everywhere.  The colour line is OpenCV 3.3's 8-bit RGB2Gray (14-bit coefficients, the
 * rounding constant folded into its table); the 16-bit line is cv_bridge's convertTo(..., CV_8U, 255. / 65535.), whose rounded float
 * product equals the integer form for all 65 536 values.  Both are written down from memory of those libraries and have not been
 * compared with them; tests/image_ref.py restates them in numpy and is the specification, csrc/image_format.h is the
 * same text for the host and the device.  Bayer patterns, 8UC3, 16UC1 and float images have no specification here.
 * lfvio_image_format_set: fmt != NULL: `image` of every later lfvio_klt_track, lfvio_track_frame and lfvio_track_frame_message points
 * to height * step bytes in that encoding (step 0: width * bytes per pixel), and everything the call does and leaves resident is, bit
 * for bit, what it does without a format on the converted image: lfvio_klt_level(ctx, 0, ...) returns the grey image, or the equalized
 * grey image.  fmt == NULL: off.  A mono8 format with step 0 or step == width is the same as none.  Off after lfvio_create; survives
 * lfvio_klt_reset and lfvio_track_frame_reset.  lfvio_clahe_apply, lfvio_gft_set_mask and lfvio_track_batch_set_mask keep taking
 * 8-bit grey.  One copy goes up as without a format, of height * step bytes; nothing more comes down.
 * lfvio_image_gray: one image in, width * height grey bytes out; fmt NULL: mono8, rows contiguous.  Touches neither the resident
 * image nor the setting.
 * lfvio_track_batch_format (with the batch calls below): the setting of the batch, one for every slot.
 * LFVIO_ERR_ARG (everything untouched): a code outside the table, step negative or above 65536; at the call that takes an image,
 * 0 < step < width * bytes per pixel; for lfvio_image_gray null ctx / pixels / out or a width or height outside [16, 8192]. */
#define LFVIO_IMG_MONO8 0
#define LFVIO_IMG_BGR8 2
#define LFVIO_IMG_RGB8 3
#define LFVIO_IMG_BGRA8 4
#define LFVIO_IMG_RGBA8 5
#define LFVIO_IMG_MONO16 6
#define LFVIO_IMG_MONO16_BE 7
#define LFVIO_IMG_MAX_STEP 65536
typedef struct { int encoding; int step; /* bytes per row; 0: width * bytes per pixel */ } LfvioImageFormat;
int lfvio_image_format_set(lfvio_ctx *ctx, const LfvioImageFormat *fmt /* NULL: mono8, rows contiguous */);
int lfvio_image_gray(lfvio_ctx *ctx, const LfvioImageFormat *fmt, int width, int height, const unsigned char *pixels,
                     unsigned char *out /* [height][width] */);

/* lfvio_track_reject / lfvio_track_undistort / lfvio_track_reset: the two steps of FeatureTracker::readImage that need the camera —
 * rejectWithF() (feature_tracker/src/feature_tracker.cpp:329-386, with myfindFundamentalMat :266-327) and undistortedPoints()
 * (:441-504) — with OCAMCamera::liftProjective (camera_model/src/camera_models/ScaramuzzaCamera.cc:623-645) on the device.
 *   the lift  of a pixel (px, py) (cv::Point2f), in double, every operation rounded on its own (nothing fused):
 *             x = (double)px - cx, y = (double)py - cy; xa = inv_scale * (x - d * y), ya = inv_scale * (-e * x + c * y) with
 *             inv_scale = 1.0 / (c - d * e), computed once on the host; phi = sqrt(xa * xa + ya * ya); z = 0, p = 1, for i = 0 .. 4:
 *             z += p * poly[i], p *= phi; P = (xa, ya, -z) (the sign is the reference's, :644).
 *   the norm  n = sqrt((P.x P.x + P.y P.y) + P.z P.z), left to right.  Eigen's own reduction may order the three terms differently
 *             and differ in the last bit; the reference does not build without Eigen and OpenCV, so the two were never compared.
 * tests/track_ref.py restates both calls in numpy and is the specification; the device gives its bits.  The C++ of
 * every lift below, the norm, P / n and the float casts of lfvio_track_undistort is lf-vio_amd/csrc/camera_models.h (with camera_kb.h),
 * one text that the kernels and the host compile.
 *   the lift of LFVIO_CAM_PINHOLE and LFVIO_CAM_MEI (PinholeCamera.cc:450-510, CataCamera.cc:556-626), in double,
 *             every operation rounded on its own, grouped as written here:
 *             host, once: inv11 = 1.0 / fx, inv13 = -cx / fx, inv22 = 1.0 / fy, inv23 = -cy / fy,
 *                         no_distortion = (k1 == 0 && k2 == 0 && p1 == 0 && p2 == 0)
 *             mx_d = inv11 * (double)px + inv13, my_d = inv22 * (double)py + inv23
 *             dist(x, y): mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2, rad = k1 * rho2 + (k2 * rho2) * rho2,
 *                         dx = (x * rad + (2.0 * p1) * mxy) + p2 * (rho2 + 2.0 * mx2),
 *                         dy = (y * rad + (2.0 * p2) * mxy) + p1 * (rho2 + 2.0 * my2)
 *             no_distortion: (mx_u, my_u) = (mx_d, my_d); otherwise eight evaluations of dist: (mx_u, my_u) = (mx_d, my_d) -
 *             dist(mx_d, my_d), then seven times (mx_u, my_u) = (mx_d, my_d) - dist(mx_u, my_u).
 *             PINHOLE: P = (mx_u, my_u, 1.0).  MEI: P = (mx_u, my_u, z) with, for xi == 1.0, z = ((1.0 - mx_u * mx_u) - my_u * my_u)
 *             / 2.0, and otherwise rho2 = mx_u * mx_u + my_u * my_u, z = 1.0 - (xi * (rho2 + 1.0)) / (xi + sqrt(1.0 + (1.0 - xi * xi)
 *             * rho2)).  Non-finite results keep IEEE semantics (the root's argument goes negative far outside the image for
 *             xi > 1).  Everything behind the lift (the norm, P / n, un_pts, the casts, the map, the velocity) is the same for
 *             all models.  tests/camera_ref.py restates these two lifts; they were never compared with the reference's Eigen build
 *             either.
 *   the lift of LFVIO_CAM_KANNALA_BRANDT (EquidistantCamera.cc:428-442 over backprojectSymmetric :716-818): the
 *             reference's MATHEMATICS — theta is the smallest non-negative real root of f(theta) = theta + k2 theta^3 + k3 theta^5 +
 *             k4 theta^7 + k5 theta^9 = r, P = (sin theta cos phi, sin theta sin phi, cos theta) — in a text of this library's own,
 *             made of + - * / sqrt floor and comparisons alone, in double, every operation rounded on its own, grouped as written:
 *             the fields: cx, cy = u0, v0; fx, fy = mu, mv; poly[0 .. 3] = k2, k3, k4, k5; nothing else is read.
 *             F(th):  t = th * th, th * (1.0 + t * (k2 + t * (k3 + t * (k4 + t * k5))))
 *             F'(th): t = th * th, 1.0 + t * (3.0 * k2 + t * (5.0 * k3 + t * (7.0 * k4 + t * (9.0 * k5))))
 *             host, once per camera: inv11 .. inv23 as for PINHOLE; theta_lim = the last point of the grid j * (pi / 4096), j = 0 ..
 *                         4096, up to which F' > 0 held at every grid point (pi if at all of them), r_lim = F(theta_lim): on
 *                         [0, theta_lim] the polynomial increases from 0, so for r <= r_lim its root there is the smallest one.
 *             x = inv11 * (double)px + inv13, y = inv22 * (double)py + inv23, r = sqrt(x * x + y * y)
 *             th = r < theta_lim ? r : theta_lim; 13 times: th = th - (F(th) - r) / F'(th), th = th < 0.0 ? 0.0 : th,
 *                         th = th > theta_lim ? theta_lim : th; theta = r <= r_lim ? th : r (beyond the monotone range and for a NaN
 *                         theta = r: the reference's own fallback when it finds no admissible root, :809-812)
 *             sin, cos:   n = floor(theta * invpio2 + 0.5), y = ((theta - n * pio2_1) - n * pio2_2) - n * pio2_2t, q = n - 4.0 *
 *                         floor(n / 4.0), all in double; z = y * y, s = y + (z * y) * (S1 + z * (S2 + .. z * S6)), c = 1.0 - (0.5 * z
 *                         - z * (z * (C1 + z * (C2 + .. z * C6)))) with fdlibm's constants (camera_kb.h); q = 1 and 3 swap s and c,
 *                         the sine is negated for q = 2 and 3, the cosine for q = 1 and 2.  Nothing is converted to an integer.
 *             r < 1e-10: cphi = 1.0, sphi = 0.0 (:722-725); otherwise cphi = x / r, sphi = y / r.  P = (s * cphi, s * sphi, c).
 *             Stated deviations: x / r, y / r in place of cos(atan2(y, x)), sin(atan2(y, x)); Newton's method in place of the
 *             companion matrix's eigenvalues; a calibration whose polynomial turns down and comes up again inside [0, pi] would
 *             give the reference a root beyond theta_lim that this lift does not look for (none of the reference's three has one),
 *             and the grid can miss a dip of F' narrower than a step.  tests/kb_ref.py restates this lift and holds it to a
 *             50-digit evaluation of the reference's definition (tests/test_kb_ref.py: the root to 3.6 eps where F' >= 0.1, sin and
 *             cos to 5.4 ulp, the bearing to 25.6 eps where F' >= 0.1); the device gives the restatement's bits.
 *   the lift of LFVIO_CAM_EQUIRECT: the camera of the EXPANDED image that lfvio_remap_build's LFVIO_MAP_EQUIRECT map
 *             writes — GetremapMat's ray (pointcloud_image_fusion.cpp:93-101) with the float pixel in place of the integer one.
 *             fx, fy carry that image's width and height (finite, integral, in [16, 8192]); no other field is read.  In double,
 *             grouped as written: lon = ((double)px / fx - 0.5) * (2.0 * pi), lat = -(((double)py / fy - 0.5) * pi),
 *             P = (cos(lat) * sin(lon), cos(lat) * cos(lon), sin(lat)), sine and cosine as the KANNALA_BRANDT lift takes them.  At an
 *             integer pixel this is the map's own ray bit for bit, so tracked bearings are in the frame the map was built in.  The
 *             lift ONLY: lfvio_cam_project, lfvio_remap_build and lfvio_cloud_fuse with LFVIO_FUSE_CAMERA refuse the model (the
 *             projection exists as LFVIO_FUSE_EQUIRECT).  tests/equirect_ref.py restates it and holds it to a 50-digit evaluation on
 *             [0, width] x [0, height] (tests/test_equirect_lift.py: to 5.438 eps max(|P|, 1), twice the 2.719 measured).
 *   the camera LFVIO_ERR_ARG of every call that takes an LfvioCamera: models 1 and 4 and any model outside {0, 2, 3, 5, 6}; for
 *             EQUIRECT fx or fy non-finite, non-integral or outside [16, 8192]; for PINHOLE
 *             and MEI a non-finite value among cx, cy, fx, fy, k1, k2, p1, p2, fx == 0 or fy == 0, and for MEI a non-finite xi; for
 *             KANNALA_BRANDT a non-finite value among cx, cy, fx, fy, poly[0 .. 3], fx == 0 or fy == 0.  An OCam camera's fx .. xi are
 *             not read, a PINHOLE or MEI camera's c, d, e, poly are not, a KANNALA_BRANDT camera's c, d, e, poly[4], k1 .. xi are
 *             not: they may be indeterminate.
 *
 * lfvio_track_reject: the bearings are P / n, a true division per component, of cur_pts (corr1) and forw_pts (corr2).  Per sample
 * set compute_E_21 and check_inliers; the first hypothesis with the largest score > 0 wins; the refit over the winner's inliers and
 * check_inliers again; that mask is status[].  compute_E_21 (:186-217) and check_inliers (:218-264) are those of
 * initial_ex_rotation.cpp: this is lfvio_two_view's arithmetic up to its mask, bit for bit on the same bearings and sample sets,
 * without the decomposition and the triangulations.  The sample sets are an INPUT, as for lfvio_two_view.
 *   out->status 0   a model was found; status[] is its mask, num_inliers its count, E the refit's.
 *   out->status 1   no hypothesis scored > 0, or the winner has fewer than 8 inliers.  status[] is all 1 (nothing is rejected), E is
 *                   untouched, best_sample and num_inliers are as lfvio_two_view reports them.  A stated deviation: the reference
 *                   throws from vector::at there.
 *   out->status 2   N < 8 (the test of :331 failing): no device work, status[] all 1, best_sample -1, num_inliers 0, best_score 0,
 *                   E and the bearing outputs untouched.
 * bearing_cur / bearing_forw (or NULL) receive the unit bearings where the device ran (status 0 and 1).
 * LFVIO_ERR_ARG (every output untouched): null ctx / in / camera / status / out, cur_pts or forw_pts null with N > 0, a camera
 * refused above, N outside [0, 4096]; with N >= 8: samples null, S outside [1, 1024], a sample index outside [0, N).
 *
 * lfvio_track_undistort: un_pts = ((float)(P.x / P.z), (float)(P.y / P.z)); un_pts_3d = (float)(P.k / n) per component.  The
 * context keeps what prev_un_pts_map_3d is: the (id, un_pts_3d) pairs of the PREVIOUS call, with std::map::insert semantics — the
 * first occurrence of an id wins; ids are taken AS PASSED, so a point that was -1 in that call is in the map under -1, even if the
 * caller numbered it afterwards, and -1 is never looked up: a new corner has zero velocity on its second frame too (the
 * reference's behaviour, restated, not repaired).  Velocity of point i: with ids[i] != -1 and the id found at index j of the
 * previous call, (float)((double)(cur_3d[i].k - prev_3d[j].k) / dt), the subtraction in float (cv::Point3f members), dt = time -
 * (the previous call's time) in double; otherwise 0.  All velocities are 0 when the map is empty: a first call, a call after
 * lfvio_track_reset, a call after a call with N = 0.  dt == 0 and non-finite pixels keep IEEE semantics.  matched (or NULL)
 * receives j, or -1.  After the call the map and the time are this call's.  A stated deviation: the reference forgets to clear
 * pts_velocity_3d in the empty-map branch; here the output has exactly N entries.
 * LFVIO_ERR_ARG (every output, the resident map and the time untouched): null ctx / in / camera, pts, ids, un_pts, un_pts_3d or
 * velocity_3d null with N > 0, a camera refused above (lfvio_track_reject), N outside [0, 4096], a NaN time.
 * All three run on the feature stream like lfvio_klt_track: they do not wait for an optimization in flight.  The two maps live in
 * device memory of their own (2 x 64 KiB, allocated at the first use), not in the feature calls' staging block. */
#define LFVIO_CAM_OCAM 0
#define LFVIO_CAM_PINHOLE 2
#define LFVIO_CAM_MEI     3   /* 1 and 4 are refused, like every model outside {0, 2, 3, 5, 6} */
#define LFVIO_CAM_KANNALA_BRANDT 5
#define LFVIO_CAM_EQUIRECT 6  /* the lift only: the expanded image of LFVIO_MAP_EQUIRECT; fx, fy = its width, height */
#define LFVIO_TRACK_MAX_POINTS 4096
typedef struct {
  int model;             /* LFVIO_CAM_OCAM, _PINHOLE, _MEI, _KANNALA_BRANDT or _EQUIRECT; anything else: LFVIO_ERR_ARG */
  double cx, cy;         /* OCam: center_x, center_y; PINHOLE: cx, cy; MEI and KANNALA_BRANDT: u0, v0 */
  double c, d, e;        /* OCam only: the affine part; inv_scale = 1.0 / (c - d * e) */
  double poly[5];        /* OCam: SCARAMUZZA_POLY_SIZE; KANNALA_BRANDT: poly[0 .. 3] = k2, k3, k4, k5 (NOT the k1, k2 below) */
  double fx, fy;         /* PINHOLE: fx, fy; MEI: gamma1, gamma2; KANNALA_BRANDT: mu, mv; EQUIRECT: width, height.  Not read for OCam, like everything below */
  double k1, k2, p1, p2; /* PINHOLE and MEI: distortion_parameters */
  double xi;             /* MEI: mirror_parameters.xi */
} LfvioCamera;
typedef struct {
  const LfvioCamera *camera;
  int num_points;          /* N, 0 .. 4096 */
  const float *cur_pts;    /* [N][2] cv::Point2f, after the flow's reduceVector */
  const float *forw_pts;   /* [N][2] */
  int num_samples;         /* S in [1, 1024]; the reference: 100 */
  const int *samples;      /* [S][8] indices into the matches */
} LfvioTrackRejectIn;
typedef struct { int status, best_sample, num_inliers; double best_score, E[9]; } LfvioTrackRejectOut;
int lfvio_track_reject(lfvio_ctx *ctx, const LfvioTrackRejectIn *in, unsigned char *status /* [N] */, LfvioTrackRejectOut *out,
                       double *bearing_cur /* [N][3] or NULL */, double *bearing_forw /* [N][3] or NULL */);
typedef struct {
  const LfvioCamera *camera;
  int num_points;      /* N, 0 .. 4096 */
  const float *pts;    /* [N][2] cur_pts */
  const int *ids;      /* [N], -1: not yet numbered */
  double time;         /* cur_time */
} LfvioTrackUndistortIn;
int lfvio_track_undistort(lfvio_ctx *ctx, const LfvioTrackUndistortIn *in, float *un_pts /* [N][2] */, float *un_pts_3d /* [N][3] */,
                          float *velocity_3d /* [N][3] */, int *matched /* [N]: index in the previous call, or -1; or NULL */);
int lfvio_track_reset(lfvio_ctx *ctx);   /* forget the resident map and time */

/* lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply / lfvio_remap_reset: the camera models the other way — spaceToPlane of the
 * four models on the device — and what the reference builds on it: the equirectangular expansion of the panoramic annular image
 * (pointcloud_image_fusion: GetremapMat, pointcloud_image_fusion.cpp:83-114, once; cv::remap(show_img, equal_rectangle_img, remap_x,
 * remap_y, 0) per BGR8 image, pointcloud_image_fusion_node.cpp:62-81) and OCAMCamera::initUndistortRectifyMap
 * (ScaramuzzaCamera.cc:723-777), the same machinery with a perspective ray per output pixel.  DESIGN.md 3w.
 *   the projection of a point P = (X, Y, Z), in double, every operation rounded on its own, grouped as written here; the C++ is
 *             cam_project of lf-vio_amd/csrc/camera_models.h over camera_atan.h, tests/project_ref.py restates it in numpy and is the
 *             specification, held to a 50-digit evaluation of the reference's definitions (tests/test_project_ref.py: OCAM to 7.98,
 *             PINHOLE to 10.78, MEI to 21.64 and, where F' >= 0.1, KANNALA_BRANDT to 30.58 eps max(|u|, |v|, 1); atan to 1.412 ulp).
 *   LFVIO_CAM_OCAM (ScaramuzzaCamera.cc:654-674): n = sqrt(X * X + Y * Y); theta = atan(-Z / n); rho = 0, t = 1, for i = 0 .. 19:
 *             rho += t * inv_poly[i], t *= theta (the reference's loop over SCARAMUZZA_INV_POLY_SIZE, not Horner); inv = 1.0 / n;
 *             xn = (X * inv) * rho, yn = (Y * inv) * rho; u = (xn * c + yn * d) + cx, v = (xn * e + yn) + cy.  atan(-Z / n) stands
 *             for the reference's atan2(-Z, n), n >= 0; at n == 0 the reference's pixel is NaN either way (0 * inf), so this is a
 *             deviation of the text, not of the value.
 *   LFVIO_CAM_PINHOLE (PinholeCamera.cc:520-542): x = X / Z, y = Y / Z; unless no_distortion: (dx, dy) = dist(x, y) of the lift
 *             above, x += dx, y += dy; u = fx * x + cx, v = fy * y + cy.
 *   LFVIO_CAM_MEI (CataCamera.cc:636-659): the same with z = Z + xi * n3 in place of Z, n3 the norm of the lift above,
 *             sqrt((X * X + Y * Y) + Z * Z).
 *   LFVIO_CAM_KANNALA_BRANDT (EquidistantCamera.cc:451-461): the reference's MATHEMATICS (theta = acos(Z / |P|), phi = atan2(Y, X),
 *             p = F(theta) (cos phi, sin phi)) in a text of this library's own: rxy = sqrt(X * X + Y * Y); q = rxy / Z, a = atan(q);
 *             theta = a for Z > 0, pi_hi + (a + pi_lo) for Z < 0 (the two parts of pi), pi / 2 for Z == 0 and rxy > 0, and q — a NaN —
 *             otherwise (the zero vector, a NaN); cphi = X / rxy, sphi = Y / rxy, and (1.0, 0.0) for rxy < 1e-10; r = F(theta);
 *             u = fx * (r * cphi) + cx, v = fy * (r * sphi) + cy.  Stated deviations: theta from the arctangent of rxy / Z in place
 *             of the arc cosine (the same angle), X / rxy, Y / rxy in place of cos(atan2(Y, X)), sin(atan2(Y, X)), and phi = 0 below
 *             rxy = 1e-10 where the reference's atan2 still follows (X, Y) (there r F(theta) < 2e-10 of a focal length).
 *   atan      s_atan.c's scheme of fdlibm in + - * /, comparisons and fabs (camera_atan.h): a = |x|; t = a below 7 / 16, (2.0 * a -
 *             1.0) / (2.0 + a) below 11 / 16, (a - 1.0) / (a + 1.0) below 19 / 16, (a - 1.5) / (1.0 + 1.5 * a) below 39 / 16 and
 *             -1.0 / a from there; z = t * t, w = z * z, s1 = z * (aT0 + w * (aT2 + .. w * aT10)), s2 = w * (aT1 + w * (aT3 + .. w *
 *             aT9)); below 7 / 16 t - t * (s1 + s2), otherwise atanhi - ((t * (s1 + s2) - atanlo) - t); negated for x < 0; x itself
 *             for a < 2^-29, +-(atanhi[3] + atanlo[3]) for a >= 2^66.  No libm call anywhere in the projection.
 *
 * lfvio_cam_project: px[k] = (u, v) of P[k], k < n.  LFVIO_ERR_ARG (px untouched): null ctx / proj / proj->camera, P or px null
 * with n > 0, a camera refused above (lfvio_track_reject), for OCam a non-finite inv_poly entry, n outside [0, 1 << 20].
 *
 * lfvio_remap_build: the float maps of a width x height OUTPUT image, map_x = (float)u, map_y = (float)v of the ray of output pixel
 * (i, j) (column, row), in double, grouped as written:
 *   LFVIO_MAP_EQUIRECT     lon = ((double)i / (double)width - 0.5) * (2.0 * pi), lat = -(((double)j / (double)height - 0.5) * pi),
 *                          P = (cos(lat) * sin(lon), cos(lat) * cos(lon), sin(lat)) (:93-101), sine and cosine as the KANNALA_BRANDT
 *                          lift takes them (above; held to 2.716 ulp on [-pi, pi] as they are, so no symmetry is applied).
 *   LFVIO_MAP_PERSPECTIVE  P = M (i, j, 1): P.k = (M[3k] * i + M[3k + 1] * j) + M[3k + 2].  A stated deviation: the reference forms
 *                          R_inv * K_rect_inv and the ray in float (Matrix3f); here the caller supplies the product, in double.
 * The maps stay resident in the context, in device memory of their own (allocated at the first build), until the next build or
 * lfvio_remap_reset; map_x / map_y (both, or both NULL) receive them.  LFVIO_ERR_ARG (outputs and the resident maps untouched):
 * null ctx / in / in->proj / camera, a projector refused above, an unknown kind, for PERSPECTIVE a non-finite M entry, width or
 * height outside [16, 8192], exactly one of map_x and map_y null.
 *
 * lfvio_remap_apply: cv::remap(src, out, map_x, map_y, INTER_NEAREST) with BORDER_CONSTANT 0 through the resident maps.  Per output
 * pixel sx = saturate_cast<short>(map_x), sy likewise: round to nearest, ties to even, clamped to [-32768, 32767]; a NaN counts as
 * outside.  With 0 <= sx < src_width and 0 <= sy < src_height the source pixel's bytes are copied, otherwise zero bytes are
 * written.  Bytes per pixel are fmt->encoding's (1, 3, 3, 4, 4, 2, 2 for LFVIO_IMG_MONO8 .. _MONO16_BE); fmt->step is the SOURCE's,
 * the output's rows are contiguous (height * width * bytes per pixel bytes); nothing is converted.  fmt NULL: mono8, rows
 * contiguous, as for lfvio_image_gray.  THIS LINE IS WRITTEN DOWN FROM MEMORY of OpenCV 3.3's RemapInvoker / remapNearest: no
 * OpenCV was at hand and nobody has compared them (tests/project_ref.py is the specification).
 * LFVIO_ERR_ARG (out untouched): null ctx / pixels / out, src_width or src_height outside [16, 8192], a format
 * lfvio_image_format_set refuses, 0 < step < src_width * bytes per pixel; and, as lfvio_klt_level without a resident image, no
 * resident map (before the first build, after lfvio_remap_reset).
 * All four run on the feature stream like lfvio_klt_track: they do not wait for an optimization in flight, and they touch neither
 * the resident image nor any setting of the tracker calls. */
#define LFVIO_OCAM_INV_POLY_SIZE 20
typedef struct {
  const LfvioCamera *camera;
  double inv_poly[LFVIO_OCAM_INV_POLY_SIZE];  /* OCam only (SCARAMUZZA_INV_POLY_SIZE); unused tail 0.0 */
} LfvioProjector;
int lfvio_cam_project(lfvio_ctx *ctx, const LfvioProjector *proj, int n, const double *P /* [n][3] */, double *px /* [n][2] */);
#define LFVIO_MAP_EQUIRECT    0  /* GetremapMat */
#define LFVIO_MAP_PERSPECTIVE 1  /* initUndistortRectifyMap */
typedef struct {
  const LfvioProjector *proj;
  int kind, width, height;  /* width, height: of the OUTPUT image */
  double M[9];              /* PERSPECTIVE only: ray = M (u, v, 1), row-major */
} LfvioRemapIn;
int lfvio_remap_build(lfvio_ctx *ctx, const LfvioRemapIn *in, float *map_x, float *map_y /* [height][width], or both NULL */);
int lfvio_remap_apply(lfvio_ctx *ctx, const LfvioImageFormat *fmt, int src_width, int src_height, const unsigned char *pixels,
                      unsigned char *out /* [height][width * bytes per pixel] of the resident map's size */);
int lfvio_remap_reset(lfvio_ctx *ctx);   /* forget the resident maps */

/* lfvio_track_source_set: track on the EXPANDED image — level 0 of the fresh pyramid gathered through the resident map.
 * All three of the reference's launch files that carry the expansion node remap its equal_rectangle_img onto /camera/image_raw
 * (mindvision.launch:28-32), so its tracker can be fed the expanded image; here the raw source image goes up once and never comes down.
 * src != NULL: `image` of every later lfvio_klt_track, lfvio_track_frame and lfvio_track_frame_message is the SOURCE image: src_height
 * rows of src_width pixels in the encoding and step of lfvio_image_format_set (mono8 with contiguous rows while that is off), and
 * in->width, in->height stay the size of the image that is TRACKED, which must be the resident map's (lfvio_remap_build).  Level 0 is
 * the grey value above of the pixel lfvio_remap_apply would have written (for an outside entry the grey value of a zero pixel), in
 * one kernel (k_remap_gray, csrc/kernels_tracksource.h); the bytes that go up are src_height * step.  The contract: every output array
 * of the three calls, and lfvio_klt_level afterwards, is bit for bit what a second context gives that is fed lfvio_remap_apply's
 * output under lfvio_image_format_set({the same encoding, step 0}).  CLAHE, the mask, detection, the table and the message see an image
 * of in->width x in->height.  The camera of such a call is the TRACKED image's: LFVIO_CAM_EQUIRECT for an LFVIO_MAP_EQUIRECT map, a
 * distortion-free LFVIO_CAM_PINHOLE for an LFVIO_MAP_PERSPECTIVE one.  The integer map is shared with lfvio_remap_apply and
 * lfvio_cloud_fuse: each rebuilds it when it finds it written for another source geometry, so they may alternate.
 * src == NULL: off.  Off after lfvio_create; survives lfvio_klt_reset, lfvio_track_frame_reset and lfvio_remap_reset.  The batched
 * route (lfvio_track_batch_*) does not look at this setting or at the resident map: it has a setting of its own
 * (lfvio_track_batch_source) and a map per slot (lfvio_track_batch_map), below.
 * LFVIO_ERR_ARG: at the set call (the setting untouched) src_width or src_height outside [16, 8192]; at the tracker call, before
 * anything is touched (the resident pyramid, the track table, the maps and the stream as they were): no resident map (never built, or
 * after lfvio_remap_reset), a resident map of another size than in->width x in->height, and what lfvio_image_format_set's check
 * refuses beside src_width x src_height (0 < step < src_width * bytes per pixel). */
typedef struct { int src_width, src_height; } LfvioTrackSource;
int lfvio_track_source_set(lfvio_ctx *ctx, const LfvioTrackSource *src /* NULL: off */);

/* lfvio_cloud_fuse: the other half of pointcloud_image_fusion — every point of a lidar scan taken into the camera frame, projected and
 * marked in the expanded image (pointcloud_image_fusion_node.cpp:92-115, in comments as shipped; laserCloudIn is pointcloud_callback's,
 * :121-125).  One copy up ([cloud | image]), the launches back to back, one copy down.  DESIGN.md 3x; tests/fuse_ref.py restates it
 * in numpy and is the specification; the C++ is fuse_point of lf-vio_amd/csrc/fuse_plan.h.
 *   the cloud   the raw `data` bytes of a sensor_msgs/PointCloud2: n points of point_step bytes, x / y / z float32 at the byte offsets
 *               off_x / off_y / off_z of a point, of the byte order big_endian says.  No alignment is required of offsets or step.
 *   per point   in double, every operation rounded on its own, grouped as written: x, y, z widened;
 *               P.k = ((R[3k] * x + R[3k + 1] * y) + R[3k + 2] * z) + T[k] (camera_R_lidar, camera_T_lidar; R row-major);
 *               r = sqrt((X * X + Y * Y) + Z * Z); the point passes the RANGE GATE iff r > 0 && r >= min_range && r <= max_range
 *               && r < inf (a NaN or infinite coordinate fails, and so does an Ouster no-return (0, 0, 0)).
 *   LFVIO_FUSE_EQUIRECT  the inverse of LFVIO_MAP_EQUIRECT: nxy = sqrt(X * X + Y * Y), dropped at nxy == 0 (the pole);
 *               a = atan(X / Y) (the atan above); lon = a for Y > 0, pi_hi + (a + pi_lo) for Y < 0 and X >= 0, (a - pi_lo) - pi_hi
 *               for Y < 0 and X < 0, +-pi / 2 by the sign of X for Y == 0: the angle of atan2(X, Y).  lat = atan(Z / nxy).
 *               fx = width * (0.5 + lon / (2.0 * pi)), fy = height * (0.5 - lat / pi); col = (int)fx, row = (int)fy (truncation, as
 *               the reference's int idx_x = ...; both >= 0); col == width (the seam lon = +pi) wraps to column 0, row == height
 *               (lat = -pi / 2 as a double: |Z / nxy| beyond about 1e16) becomes height - 1.  Stated deviations: the reference
 *               normalises and takes asin(z), the same angle (the treatment KANNALA_BRANDT's acos got); and at row == height the
 *               reference writes outside its image.
 *   LFVIO_FUSE_CAMERA    (u, v) = the projection above of P through proj; col, row = saturate_cast<short> of (float)u, (float)v
 *               as lfvio_remap_apply rounds; kept iff 0 <= col < width and 0 <= row < height and, because a projection through the
 *               centre otherwise yields plausible pixels, PINHOLE: Z > 0, MEI: Z + xi * r > 0.
 *   the image   image_mode LFVIO_FUSE_IMAGE_NONE; _GIVEN: pixels is a width x height image of fmt (fmt->step its row's bytes);
 *               _REMAP: pixels is a src_width x src_height image of fmt that goes through the RESIDENT maps first, exactly as
 *               lfvio_remap_apply takes it (same integer map, same rebuild decision): a resident map of width x height is required.
 *               fmt NULL: mono8, rows contiguous.  With paint_on nonzero the first bytes-per-pixel bytes of paint are written at
 *               every marked pixel (the reference: (255, 0, 0) into bgr8).
 * Outputs, each NULL or written: index[k] = row * width + col, or -1 for a dropped point; range = the smallest (float)r of the points
 * on a pixel, +inf where there is none (an atomic minimum on the bit pattern: positive floats order as their bits, so the order of
 * arrival does not show); colour[k] = the image's bytes at index[k] BEFORE anything is painted, zero bytes for -1; image_out = the
 * (remapped) image, rows contiguous, painted when paint_on (sampling and painting are two launches in stream order); counts =
 * (points kept, dropped by the range gate, dropped by the projection).
 * LFVIO_ERR_ARG (every output untouched, the resident maps still serving the next lfvio_remap_apply): null ctx / in / out; n outside
 * [0, 1 << 20] or a null cloud with n > 0; point_step outside [12, 1024]; an offset outside [0, point_step - 4] or two fields that
 * overlap; big_endian not 0 or 1; a non-finite R or T entry; min_range negative or not finite, max_range below min_range or NaN; an
 * unknown kind; width or height outside [16, 8192]; for CAMERA a projector lfvio_cam_project refuses; an unknown image_mode; with an
 * image: null pixels, a format lfvio_image_format_set refuses, 0 < step < the row's bytes, for REMAP src_width or src_height outside
 * [16, 8192]; colour or image_out without an image; REMAP without a resident map or with one of another size (as lfvio_remap_apply).
 * Runs on the feature stream like lfvio_remap_apply: it does not wait for an optimization in flight and touches no tracker state. */
#define LFVIO_FUSE_EQUIRECT 0
#define LFVIO_FUSE_CAMERA   1
#define LFVIO_FUSE_IMAGE_NONE  0
#define LFVIO_FUSE_IMAGE_GIVEN 1
#define LFVIO_FUSE_IMAGE_REMAP 2
#define LFVIO_FUSE_MAX_POINTS (1 << 20)
typedef struct {
  const unsigned char *cloud;      /* n * point_step bytes */
  int n, point_step, off_x, off_y, off_z, big_endian;
  double R[9], T[3];               /* P = R p + T, R row-major */
  double min_range, max_range;     /* max_range may be +inf */
  int kind, width, height;         /* width, height: of the image the points are marked in */
  const LfvioProjector *proj;      /* CAMERA only */
  int image_mode;
  const LfvioImageFormat *fmt;     /* NULL: mono8, rows contiguous */
  int src_width, src_height;       /* REMAP only */
  const unsigned char *pixels;     /* GIVEN: height rows; REMAP: src_height rows */
  int paint_on;
  unsigned char paint[4];
} LfvioFuseIn;
typedef struct {                   /* each NULL, or written */
  int *index;                      /* [n] */
  float *range;                    /* [height][width] */
  unsigned char *colour;           /* [n][bytes per pixel] */
  unsigned char *image_out;        /* [height][width * bytes per pixel] */
  int *counts;                     /* [3]: kept, dropped by the gate, dropped by the projection */
} LfvioFuseOut;
int lfvio_cloud_fuse(lfvio_ctx *ctx, const LfvioFuseIn *in, LfvioFuseOut *out);

/* lfvio_track_frame / lfvio_track_frame_reset: one image through FeatureTracker::readImage (feature_tracker/src/feature_tracker.cpp:
 * 95-184) and the node's updateID loop (feature_tracker_node.cpp:102-111) in ONE call: one copy up ([sample_words | image]), the
 * stages below enqueued back to back, one copy down.  The track table (cur_pts, ids, track_cnt) is resident in the context, and so
 * is n_id; the counts between the stages stay on the device.  The stages are those of the separate calls above, on the same
 * kernels and the same resident state — the pyramid of lfvio_klt_track, the base mask of lfvio_gft_set_mask, the setting of
 * lfvio_clahe_set, the (id, un_pts_3d) map and time of lfvio_track_undistort — and every one of these is left as the separate calls
 * would have left it: a caller may mix the two routes (the table itself is only ever filled by this call).
 *   1  the flow (lfvio_klt_track, the inBorder test included) from the resident table's points
 *   2  cur, forw, ids and track_cnt keep the entries with status 1, in order (reduceVector); track_cnt += 1; n1 are left
 *   3  publish != 0: the sample sets are drawn ON THE DEVICE, which alone knows n1, from the caller's words: for set s and k = 0 .. 7
 *      r = sample_words[s][k] % (n1 - k); for every index c already chosen for this set, in ascending order, if (r >= c) r++;
 *      samples[s][k] = r — eight distinct indices in [0, n1).  Then lfvio_track_reject on them (n1 < 8: nothing is drawn, status 2)
 *      and reduceVector by its mask; n2 are left
 *   4  publish != 0: lfvio_gft_detect; the table becomes [forw[kept] | corners], the corners with id -1 and count 1
 *   5  lfvio_track_undistort on the table's points with the ids AS THEY ARE NOW, the -1 included (the quirk stated there is kept)
 *   6  every id that is -1 takes the next n_id, in index order; num_new were numbered
 * out: the scalars, `reject` and `detect` (all zero with publish == 0; reject.E is zero unless reject.status is 0), and the table
 * with the outputs of step 5 in the caller's arrays of `capacity` entries, num_points written.  stages (or NULL), every pointer in it
 * (or NULL) an array of `capacity` entries (samples: num_samples x 8): next_pts and status of the flow for the points the call began
 * with, the sample sets as drawn (written where n1 >= 8), the rejection mask [num_tracked], kept [detect.num_kept] and corners
 * [detect.num_corners][2].
 * tests/track_frame_ref.py restates the mapping of step 3 and the frame; the device gives its bits.
 * LFVIO_ERR_ARG (every output, the table, n_id, the resident image, the map and the time untouched): null ctx / in / out / image /
 * camera / an array of out, null sample_words with publish != 0, a field outside the range that the separate call states for it, a
 * camera that lfvio_track_reject refuses, num_samples outside [1, 1024], capacity < max(max_count, the table's count) or > 4096, a NaN
 * time, with publish != 0 a base mask that is not the image's size.  A call that fails later changes nothing either: the table, like
 * the pyramid and the map, is double-buffered and swapped when the call has succeeded.  Runs on the feature stream like
 * lfvio_klt_track: it does not wait for an optimization in flight.
 * lfvio_track_frame_reset: lfvio_klt_reset and lfvio_track_reset, the table empty and n_id = 0. */
typedef struct {
  int width, height;                /* as LfvioKltIn */
  const unsigned char *image;
  double time;                      /* cur_time; not NaN */
  int publish;                      /* PUB_THIS_FRAME: 0 skips steps 3 and 4 */
  const LfvioCamera *camera;
  int win_size, max_level, max_iterations;   /* as LfvioKltIn */
  double epsilon, min_eig_threshold;
  int border;
  int max_count;                    /* as LfvioGftIn */
  double quality_level;
  int min_distance, mask_radius;
  int num_samples;                  /* S in [1, 1024]; the reference: 100 */
  const unsigned int *sample_words; /* [S][8] uniform 32-bit words; may be NULL with publish == 0 */
  int capacity;                     /* entries of each array of out and stages: max(max_count, the table's count) .. 4096 */
} LfvioTrackFrameIn;
typedef struct {
  int num_points, num_new, levels_used, num_tracked /* n1 */, num_after_reject /* n2; = n1 with publish == 0 */;
  LfvioTrackRejectOut reject;
  LfvioGftOut detect;
  float *pts;          /* [capacity][2] cur_pts after the call */
  int *ids;            /* [capacity], numbered */
  int *track_cnt;      /* [capacity] */
  float *un_pts;       /* [capacity][2] */
  float *un_pts_3d;    /* [capacity][3] */
  float *velocity_3d;  /* [capacity][3] */
} LfvioTrackFrameOut;
typedef struct {
  float *next_pts;        /* [capacity][2] */
  unsigned char *status;  /* [capacity] */
  int *samples;           /* [S][8] */
  unsigned char *mask;    /* [capacity] */
  int *kept;              /* [capacity] */
  float *corners;         /* [capacity][2] */
} LfvioTrackFrameStages;
int lfvio_track_frame(lfvio_ctx *ctx, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, const LfvioTrackFrameStages *stages /* or NULL */);
int lfvio_track_frame_reset(lfvio_ctx *ctx);

/* lfvio_track_frame_message: lfvio_track_frame — the same checks, stages and resident state afterwards, the same bits in out and
 * stages — and, with in->publish != 0, the feature message the node builds behind readImage (feature_tracker_node.cpp:113-170), built
 * on the device by one more kernel behind undistortedPoints and brought down in the same block: no second copy, no second wait.
 * One row for every table entry i with track_cnt[i] > 1, in table order, the nine floats of a type-2 trace record (host/replay.h):
 *   un_pts_3d[i].x, .y, .z | (float)(ids[i] * NUM_OF_CAM + 0), NUM_OF_CAM = 1, rounded to nearest even | pts[i].x, .y |
 *   velocity_3d[i].x, .y, .z
 * with the numbered ids of step 6.  rows has in->capacity rows.  publish == 0: nothing more is launched, num_rows = 0, rows untouched.
 * Whether the message goes out (the FREQ gate, the skipped first publication) is the caller's: host/image_gate.h.
 * LFVIO_ERR_ARG as lfvio_track_frame, and for a null msg or msg->rows; everything, msg included, untouched. */
typedef struct {
  int num_rows;
  float *rows; /* [capacity][9] */
} LfvioTrackMessage;
int lfvio_track_frame_message(lfvio_ctx *ctx, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, const LfvioTrackFrameStages *stages /* or NULL */,
                              LfvioTrackMessage *msg);

/* lfvio_track_batch_*: many image streams through lfvio_track_frame_message in ONE call.  A SLOT is one stream's resident tracker
 * state — everything a context holds for the single route: the two pyramid buffers and the resident image's size, the base mask, the
 * detector's arrays, the two track tables with n_id and the count, the two (id, un_pts_3d) maps and the time.  The slots are the
 * batch's own: the calls above never touch a slot, and the calls below never touch the state of the calls above.  A batch call makes
 * the launches of ONE frame, each with the slot as the third grid dimension, one copy up ([slot descriptors | sample_words of the
 * publishing slots | images]) and one copy down, whatever the number of slots.
 * THE CONTRACT: after any sequence of batch calls, slot i's outputs (LfvioTrackFrameOut with its arrays, and the message) and its
 * resident state are, bit for bit, those of a fresh context given slot i's active frames, in order, through
 * lfvio_track_frame_message with the same base mask and CLAHE setting.  The kernels run the single route's device functions.
 * There are no `stages` here: lfvio_track_frame remains the route for looking inside a frame.
 *   lfvio_track_batch_reserve   slots in [1, 64]; 0 frees the batch's memory.  Every slot is empty afterwards, as a fresh context is
 *                               (no image, no mask, an empty table, n_id = 0); the CLAHE setting, which is the batch's, stays.  An
 *                               allocation that fails is LFVIO_ERR_DEVICE and leaves the previous reservation usable.
 *   lfvio_track_batch_set_mask  lfvio_gft_set_mask for one slot, or for every slot with slot = -1.  pixels NULL: all 255 again.
 *   lfvio_track_batch_clahe     lfvio_clahe_set for the batch: one setting for every slot.  NULL: off.
 *   lfvio_track_batch_format    lfvio_image_format_set for the batch: one setting for every slot, and the contract above holds with
 *                               the converted images.  NULL: off.  A step below width * bytes per pixel refuses the frame call.
 *   lfvio_track_batch_frame     count must be the reserved slot count; entry i is slot i.  in[i].image == NULL: slot i is idle in
 *                               this call — its state is untouched, out[i] is written with zero scalars (everything in front of the
 *                               arrays) and nothing else, msg[i].num_rows = 0.  The active entries must agree on width, height,
 *                               win_size, max_level, max_iterations, epsilon, min_eig_threshold, border, max_count, quality_level,
 *                               min_distance, mask_radius, num_samples and capacity; they may differ in image, time, publish, camera
 *                               and sample_words.  Every rule of lfvio_track_frame holds for every active entry, with that slot's
 *                               table count and that slot's base mask.  A slot with no resident image, or one of another size,
 *                               treats its image as both images.  msg: [count], every active entry's rows an array of capacity
 *                               rows; or NULL for no messages.  All entries idle: accepted, nothing is launched.
 *                               ATOMIC over the batch: a refused call (LFVIO_ERR_ARG), a call that fails later and a call that
 *                               reads a count from the device beyond its bound leave every out, every msg and every slot untouched;
 *                               the double buffers of all active slots are swapped only after the one download has been checked.
 *   lfvio_track_batch_reset     lfvio_track_frame_reset for one slot, or for every slot with slot = -1 (the base masks and the maps
 *                               stay).
 *   lfvio_track_batch_map       lfvio_remap_build for one slot, or for every slot with slot = -1 (the same recipe in each, one launch):
 *                               the slot's resident remap, built on the device, with lfvio_remap_build's checks.  The maps are the
 *                               batch's own: no batch call reads or writes the context's resident map, and lfvio_remap_*,
 *                               lfvio_cloud_fuse and the single route never touch a slot's.  Slots may hold maps of different kinds,
 *                               cameras, M and sizes.  in NULL: the slot's map (or every map) is forgotten.  After
 *                               lfvio_track_batch_reserve no slot has a map.  12 bytes per output pixel and slot, every slot with the
 *                               capacity of the largest map built; an allocation that fails is LFVIO_ERR_DEVICE and leaves the
 *                               previous maps usable.
 *   lfvio_track_batch_source    lfvio_track_source_set for the batch: one setting for every slot; it survives reserve and reset.
 *                               NULL: off.  src_width or src_height outside [16, 8192]: LFVIO_ERR_ARG, the setting untouched.  While
 *                               it is on, every active in[i].image of lfvio_track_batch_frame is the SOURCE image — src_height rows
 *                               of `step` bytes in the encoding of lfvio_track_batch_format (mono8 with contiguous rows while that is
 *                               off) — and level 0 of slot i's fresh pyramid is gathered from it through slot i's own map, all slots
 *                               in one launch (k_remap_gray_b); width and height stay the size that is TRACKED and stay under the
 *                               agreement rule.  THE CONTRACT then reads: slot i equals, bit for bit (outputs, message and every
 *                               pyramid level), a fresh context given lfvio_remap_build with slot i's recipe, lfvio_image_format_set
 *                               and lfvio_track_source_set with the batch's settings, and slot i's active frames.  The frame call
 *                               is refused (LFVIO_ERR_ARG, atomically as above: every out, msg, slot and map as it was) when an
 *                               active slot has no map, when an active slot's map is of another size than width x height, and for
 *                               what lfvio_track_batch_format's check refuses beside src_width x src_height (0 < step < src_width *
 *                               bytes per pixel).  Idle slots need no map.  The source geometry (width, height, step, bytes per
 *                               pixel) is the batch's: a frame call of another geometry than the last rewrites the integer maps of
 *                               all mapped slots in one launch first; a steady stream never does.
 *   lfvio_track_batch_level     lfvio_klt_level for one slot: level `level` of slot's resident pyramid.
 * LFVIO_ERR_ARG besides: a slot index outside [-1, slots), any call but reserve with no slots reserved.  The calls run on the feature
 * stream like lfvio_track_frame: they do not wait for an optimization in flight.   */
#define LFVIO_TRACK_BATCH_MAX_SLOTS 64
int lfvio_track_batch_reserve(lfvio_ctx *ctx, int slots);
int lfvio_track_batch_set_mask(lfvio_ctx *ctx, int slot /* -1: every slot */, int width, int height, const unsigned char *pixels /* NULL: all 255 */);
int lfvio_track_batch_clahe(lfvio_ctx *ctx, const LfvioClaheIn *cfg /* NULL: off */);
int lfvio_track_batch_format(lfvio_ctx *ctx, const LfvioImageFormat *fmt /* NULL: mono8, rows contiguous */);
int lfvio_track_batch_frame(lfvio_ctx *ctx, int count, const LfvioTrackFrameIn *in /* [count] */, LfvioTrackFrameOut *out /* [count] */,
                            LfvioTrackMessage *msg /* [count], or NULL */);
int lfvio_track_batch_reset(lfvio_ctx *ctx, int slot /* -1: every slot */);
int lfvio_track_batch_map(lfvio_ctx *ctx, int slot /* -1: every slot */, const LfvioRemapIn *in /* NULL: forget */);
int lfvio_track_batch_source(lfvio_ctx *ctx, const LfvioTrackSource *src /* NULL: off */);
int lfvio_track_batch_level(lfvio_ctx *ctx, int slot, int level, int *width, int *height, unsigned char *pixels /* or NULL: the size alone */);

/* ---- landmark-sharded API (multi-GPU) ------------------------
 * Every rank passes the same window but linearizes only landmarks [lm_begin, lm_end) (caller order);
 * IMU factors and the prior are added on the rank(s) with add_pose_side != 0 — exactly one rank.
 * The library exposes a device exchange buffer of lfvio_shard_exchange_len() doubles,
 *   [ H_pp packed | g_p | Schur sums | 16 scalars ],  scalars at lfvio_shard_scalar_offset();
 * the CALLER sum-all-reduces it in place (RCCL) where a phase function returns 1:
 *   while (state != 2) {
 *     if (lfvio_shard_linearize(ctx) == 1) all_reduce(buf[0 : len]);            // 151 KB
 *     if (lfvio_shard_solve(ctx)     == 1) all_reduce(buf[scalar_offset : len]); // 128 B
 *     if (lfvio_shard_candidate(ctx) == 1) all_reduce(buf[scalar_offset : len]); // 128 B
 *     lfvio_shard_decide(ctx, &state);   // identical decision on every rank, no broadcast
 *   }
 *   if (lfvio_shard_marg_linearize(ctx, flag) == 1) all_reduce(buf[0 : len]);   // optional: the next prior
 *   lfvio_shard_marg_finish(ctx, flag, &prior);   // identical on every rank (estimator.cpp:833-1005)
 *   lfvio_shard_finish(ctx, &sol);       // pose-side state replicated; inv_depth: own range only;
 *                                        // after the marginalization calls: the state after double2vector()
 */
int lfvio_shard_begin(lfvio_ctx *ctx, const LfvioWindow *in, int lm_begin, int lm_end, int add_pose_side);
int lfvio_shard_exchange_len(void);
int lfvio_shard_scalar_offset(void);
double *lfvio_shard_exchange_ptr(lfvio_ctx *ctx);
int lfvio_shard_linearize(lfvio_ctx *ctx);
int lfvio_shard_solve(lfvio_ctx *ctx);
int lfvio_shard_candidate(lfvio_ctx *ctx);
/* *state: 0 = linearize next, 1 = step rejected (only a new candidate), 2 = terminated */
int lfvio_shard_decide(lfvio_ctx *ctx, int *state);
/* Stream-ordered form of the same loop (RCCL is stream-ordered: make lfvio_stream(ctx) the collective's stream).  One
 * pass is ALWAYS the same seven calls, no host synchronisation in between:
 *   lfvio_shard_enqueue(ctx, 0); all_reduce(buf[0 : len]);
 *   lfvio_shard_enqueue(ctx, 1); all_reduce(buf[scalar_offset : len]);
 *   lfvio_shard_enqueue(ctx, 2); all_reduce(buf[scalar_offset : len]);
 *   lfvio_shard_enqueue(ctx, 3);                        // decision + a 64-byte flag record to pinned memory
 * and lfvio_shard_poll() waits for the oldest record not yet read (returns 1 and the state of lfvio_shard_decide, 0 when
 * nothing is outstanding, < 0 on error), so one pass can be kept in flight behind the decision being read; a pass enqueued
 * behind a terminated loop does nothing.  lfvio_shard_restart() re-arms the resident shard from its uploaded state. */
int lfvio_shard_restart(lfvio_ctx *ctx);
int lfvio_shard_enqueue(lfvio_ctx *ctx, int phase);
int lfvio_shard_poll(lfvio_ctx *ctx, int *state);
int lfvio_shard_marg_linearize(lfvio_ctx *ctx, int flag);
int lfvio_shard_marg_finish(lfvio_ctx *ctx, int flag, LfvioPrior *out);
int lfvio_shard_finish(lfvio_ctx *ctx, LfvioSolution *out);

/* ---- multi-GPU groups: the 8-GPU path behind the C-ABI (SURVEY §8b `lfvio_create(int device_mask)`, §8e) -------------
 * The host side is C++ and the collective is RCCL (ncclAllReduce on each context's own stream), called by the library
 * itself; librccl is dlopen()ed when the first group is created (LFVIO_RCCL_LIB overrides the search), so a single-GPU
 * caller has no RCCL dependency.  Three ways to form a group:
 *   lfvio_group_create(mask)       ONE process (the ROS node: estimator.cpp:484 runs on one thread under m_estimator):
 *                                  one context + stream per device whose bit is set, ncclCommInitAll
 *   lfvio_group_create_rank(...)   one process per GPU (torchrun / mpirun): ncclCommInitRank; rank 0 obtains the id from
 *                                  lfvio_group_unique_id() and the launcher broadcasts its 128 bytes
 *   lfvio_group_create_local(...)  `shards` ranks on ONE device, the all-reduce a device-side sum in rank order instead
 *                                  of RCCL — for tests of the sharded window on a one-GPU box, and the form of choice for a
 *                                  resident BATCH that fills the device: two contexts take half of the windows each
 *                                  (lfvio_group_batch_*, no collective) and their streams run side by side
 * lfvio_group_solve() is what the re-implemented Estimator::optimization() calls in place of lfvio_solve() +
 * lfvio_marginalize(): every rank is handed the same window, rank r linearizes a contiguous landmark range balanced on
 * observation count (IMU factors and prior on rank 0), per trust-region pass the ranks sum-all-reduce
 * [H_pp | g_p | Schur sums | scalars], every rank solves the identical reduced system (no broadcast, identical
 * decisions), and the marginalization costs one more all-reduce; solution and prior come out identical on every rank,
 * sol->inv_depth complete.  Same error convention as the single-context calls; lfvio_group_last_error() has the text. */
#define LFVIO_UNIQUE_ID_BYTES 128
typedef struct lfvio_group lfvio_group;
lfvio_group *lfvio_group_create(unsigned device_mask);
int lfvio_group_unique_id(char id[LFVIO_UNIQUE_ID_BYTES]);
lfvio_group *lfvio_group_create_rank(int device, int rank, int world, const char id[LFVIO_UNIQUE_ID_BYTES]);
lfvio_group *lfvio_group_create_local(int device, int shards);
void lfvio_group_destroy(lfvio_group *g);
const char *lfvio_group_last_error(const lfvio_group *g);
int lfvio_group_size(const lfvio_group *g);     /* ranks of the group                       */
int lfvio_group_local(const lfvio_group *g);    /* contexts (ranks) held by this process    */
int lfvio_group_rank(const lfvio_group *g);     /* rank of the first local context          */
lfvio_ctx *lfvio_group_ctx(lfvio_group *g, int i); /* i-th local context (any single-context call may be made on it) */
const char *lfvio_group_backend(const lfvio_group *g); /* path of the RCCL library in use, or "local" */
/* optimization() of one window, landmark-sharded: upload + optimize + download, or the three steps on their own (the
 * window stays resident: lfvio_group_optimize() may be repeated, which is what bench.py times).  marg_flag < 0: the
 * trust-region solve only. */
/* One process per GPU (lfvio_group_create_rank): these calls contain collectives, and a collective completes only when every
 * rank of the group has entered it.  All ranks must therefore make the same sequence of lfvio_group_* calls with the same
 * window, the same marg_flag and the same choice of sol == NULL / != NULL (sol->inv_depth may be NULL on some ranks and not
 * on others: the gather of the inverse depths runs either way).
 * Collectives of lfvio_group_optimize(): per pass of the trust-region loop TWO sum-all-reduces — the reduced system (only what
 * shards over landmarks: the camera part of H_pp and of g_p, the Schur sums, 16 scalars and 256 partial sums: lfvio_group_payload_doubles() = 6 886
 * doubles, 55 KB; the speed / bias rows come from the IMU factors and the prior, which every rank evaluates for itself) and the
 * 16 scalars behind the candidate (its cost and the model terms; the landmark parts of the Gauss-Newton step's norms, which the dogleg
 * needs in between, every rank forms itself from the reduced Schur sums) — and one more
 * of the reduced system for the marginalization: 2 x passes + 1 (round 4: 3 x passes + 1 of the whole 151 KB buffer).
 * A rank that fails locally inside lfvio_group_optimize() (an enqueue refused, a HIP error) does NOT leave the others waiting: it
 * enqueues no more work but keeps issuing every collective of the sequence with an error word raised in its scalars; every rank
 * reads that word behind the pass's last reduction, ends its loop in the same pass and returns LFVIO_ERR_DEVICE (the failed rank:
 * its own error).  The group stays usable.  What this cannot cover: a rank whose device or RCCL communicator is gone (its
 * collectives cannot be issued at all), and errors before the first collective that are not common to all ranks (a malformed
 * window is refused by every rank alike; an allocation failure on one rank is not) — there the caller must still treat the
 * error as fatal for the group on every rank: RCCL has no timeout of its own. */
int lfvio_group_solve(lfvio_group *g, const LfvioWindow *in, int marg_flag, LfvioSolution *sol, LfvioPrior *prior);
int lfvio_group_upload(lfvio_group *g, const LfvioWindow *in);
int lfvio_group_optimize(lfvio_group *g, int marg_flag);
int lfvio_group_download(lfvio_group *g, LfvioSolution *sol, LfvioPrior *prior);
int lfvio_group_range(const lfvio_group *g, int rank, int *lm_begin, int *lm_end); /* landmark range of a rank */
int lfvio_group_last_passes(const lfvio_group *g);      /* passes / collectives of the last lfvio_group_optimize() */
int lfvio_group_last_collectives(const lfvio_group *g);
int lfvio_group_payload_doubles(void);                  /* doubles per rank in the all-reduce of a pass's reduced system: the camera part
                                                          * of H_pp and g_p, the Schur sums, 16 scalars, 256 partial sums (55 KB; the speed / bias rows do not travel) */
/* independent resident windows split over the devices of this process (BASELINE "512 independent windows"): slot s
 * lives on local context s % lfvio_group_local(); no data-path collective */
int lfvio_group_batch_reserve(lfvio_group *g, int batch, int max_landmarks, int max_observations);
int lfvio_group_batch_upload(lfvio_group *g, int slot, const LfvioWindow *in);
int lfvio_group_batch_optimize(lfvio_group *g, int count, int marg_flag);
int lfvio_group_batch_download(lfvio_group *g, int slot, LfvioSolution *sol, LfvioPrior *prior);

#ifdef __cplusplus
}
#endif
#endif /* LFVIO_H */
