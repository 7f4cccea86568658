// window_estimator.h — host side of the drop-in, shaped for the device it feeds.
//
// The reference keeps the sliding window in `Estimator` as eleven parallel arrays that slideWindow() shuffles element by
// element (estimator.cpp:1011-1105), the landmarks as a std::list<FeaturePerId> of std::vector<FeaturePerFrame>
// (feature_manager.h:18-71) that every call walks and re-packs, and integrates every IMU sample on the host as it
// arrives (integration_base.h:29-158).  Here:
//   * FrameRing        — the eleven keyframes live in a ring: a MARGIN_OLD slide is one index increment, nothing moves;
//   * TrackTable       — landmarks are rows of ONE flat table, nine doubles per observation, eleven observation rows per
//                        track addressed through a per-track ring offset: dropping the oldest observation of every track
//                        (removeBack) moves no data either, lookups by feature id are a hash probe instead of the
//                        reference's linear std::find_if per feature, and the CSR arrays of LfvioWindow are produced by
//                        one linear pass of memcpy-sized copies into a staging block that is reused from call to call;
//   * ImuSpan          — raw samples are only buffered; the pre-integration of the spans that changed (normally the
//                        newest one) happens on the device in ONE lfvio_preintegrate call when optimization() needs it,
//                        so no 15x15 products run on the host at all.
// The functions the hot path's contract names stay what they are: vector2double() / double2vector() (a2, bit-exact on
// the host) and optimization() (a1) keep the reference's names and semantics; everything else is named for what it does,
// and INTEGRATION.md maps the reference's members onto it.
#pragma once
#include <chrono>
#include <random>
#include <unordered_map>
#include <vector>

#include "../../include/lfvio.h"
#include "small_eigen.h"

namespace lfvio {

constexpr int WINDOW_SIZE = LFVIO_WINDOW_SIZE;
constexpr int FRAMES = LFVIO_NUM_FRAMES;
constexpr double FOCAL_LENGTH = 160.0;  // parameters.h:11

// parameters.cpp / the YAML file: one process-wide record, like the reference's globals
struct Config {
  double acc_n = 0.02, gyr_n = 0.01, acc_w = 0.04, gyr_w = 0.001;  // mindvision.yaml:138-141
  double gravity[3] = {0.0, 0.0, 9.81007};                         // :142
  double solver_time = 0.04, init_depth = 5.0;                     // parameters.cpp:133, 116
  int num_iterations = 8, estimate_extrinsic = 1, estimate_td = 1;  // :134, :83, :151
  double td = -0.008, tr = 0.0, row = 960.0;
  double min_parallax = 10.0 / FOCAL_LENGTH;                       // keyframe_parallax / FOCAL_LENGTH, parameters.cpp:56-57
  // configured extrinsic (TIC / RIC, parameters.cpp:88-112): what setParameter() restores after every reset
  double tic[3] = {0, 0, 0};
  double ric[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  // HIP devices the estimator may use: bit d = device d.  One bit (default: device 0): a single context.  Several bits: an
  // lfvio_group over them — optimization() becomes ONE lfvio_group_solve(), the window's landmarks sharded over the
  // devices with RCCL all-reduces inside the library (include/lfvio.h; SURVEY §8b lfvio_create(device_mask), §8e).
  unsigned device_mask = 1u;
  // > 1: the group is `local_shards` ranks on the FIRST device of the mask (lfvio_group_create_local: the collective a
  // device-side sum) — how a one-GPU box runs the multi-rank path of the estimator end to end (tests)
  int local_shards = 0;
  // optimization() on one device returns with the state as soon as solve + gauge fix are out and lets the marginalization
  // finish in the background (lfvio_batch_optimize_begin / _finish): the pose is published ~0.2 ms earlier, the prior is
  // collected when the next window is packed.  false: the call returns when the prior is on the host as well.
  bool split_call = true;
  // ... and the next window takes that prior over ON THE DEVICE (lfvio_batch_upload_chained_device): the upload goes out behind the
  // marginalization without waiting for it, the prior never crosses PCIe.  The host's copy (`prior`) is then only refreshed when
  // something asks for it (collectPrior()).  false: the upload collects the prior and sends it back up (lfvio_batch_upload_chained).
  bool device_chain = true;
  // ESTIMATE_EXTRINSIC == 2: the two-view RANSAC of every image draws `ransac_iterations` sample sets (the reference: 100,
  // initial_ex_rotation.cpp:171).  ransac_seed == 0 seeds the generator from std::random_device like the reference
  // (random_array.cc:12-19); any other value makes the draws, and with them the calibration, reproducible.
  int ransac_iterations = 100;
  unsigned ransac_seed = 0;
  // initialStructure() without any record from outside: a full-window image for which no bootstrap record, SfM result, SfM structure
  // or relative pose was set runs relativePose() on the device (WindowEstimator::relativePose) and goes on from its result.  false:
  // such an image slides the window, as it always did.
  bool self_relative_pose = false;
};
Config &config();

// yaw / pitch / roll in DEGREES (utility.h:66-113)
Vector3d yawPitchRollDeg(const Matrix3d &R);
Matrix3d fromYawPitchRollDeg(const Vector3d &ypr);

struct FrameRing {
  int head = 0;
  int phys(int logical) const { return (head + logical) % FRAMES; }
  void advance() { head = (head + 1) % FRAMES; }
};

struct Keyframe {
  Vector3d P, V, Ba, Bg;
  Matrix3d R;
  double stamp = 0;
};

// IMU samples between two keyframes + the IntegrationBase fields the device made of them
struct ImuSpan {
  bool present = false;  // the reference's pre_integrations[i] != nullptr
  bool dirty = false;    // `pre` is stale: samples or linearization biases changed since the last device call
  std::vector<double> dt, acc, gyr;  // n | 3n | 3n
  double acc0[3] = {0, 0, 0}, gyr0[3] = {0, 0, 0}, lin_ba[3] = {0, 0, 0}, lin_bg[3] = {0, 0, 0};
  double sum_dt = 0;
  LfvioPreintegration pre;
  void open(const Vector3d &a0, const Vector3d &g0, const Vector3d &ba, const Vector3d &bg);
  void push(double d, const double *a, const double *g);
  void close() {
    present = dirty = false;
    dt.clear(), acc.clear(), gyr.clear();
    sum_dt = 0;
  }
  int samples() const { return (int)dt.size(); }
};

// One row per observation: bearing xyz, pixel uv, bearing velocity xyz (the 8-vector of estimator_node.cpp:308), cur_td
constexpr int OBS_W = 9;

class TrackTable {
 public:
  void clear();
  int live() const { return (int)order_.size(); }
  // slots in insertion order (the reference's list order)
  const std::vector<int> &order() const { return order_; }
  int id(int s) const { return id_[s]; }
  int start(int s) const { return start_[s]; }
  int count(int s) const { return count_[s]; }
  double depth(int s) const { return depth_[s]; }
  void setDepth(int s, double d) { depth_[s] = d; }
  int solveFlag(int s) const { return flag_[s]; }
  void setSolveFlag(int s, int f) { flag_[s] = f; }
  const double *obs(int s, int k) const { return &rows_[((size_t)s * FRAMES + (first_[s] + k) % FRAMES) * OBS_W]; }
  bool solvable(int s) const { return count_[s] >= 2 && start_[s] < WINDOW_SIZE - 2; }  // feature_manager.cpp:36
  int solvableCount() const;

  int find(int feature_id) const;
  int create(int feature_id, int start_frame);
  void append(int s, const double *pt8, double cur_td);

  // getCorresponding (feature_manager.cpp:118-137): the bearings of every track seen in both frames l and r, list order;
  // bl / br receive 3 doubles per match; returns the number of matches
  int corresponding(int l, int r, std::vector<double> *bl, std::vector<double> *br) const;
  // feature_manager.cpp:45-95: the frame's observations (ids ascending, first occurrence of an id wins) are appended;
  // returns the number of continued tracks
  int appendFrame(int frame_count, int n, const int *ids, const double *pts8, double td);
  // feature_manager.cpp:353-369 summed over the tracks seen in both of the two frames before the newest one
  void parallax(int frame_count, double *sum, int *num) const;
  // feature_manager.cpp:312-330 / 271-310: every track loses its frame-0 observation and moves one frame down; with
  // `survivors` the tracks that started in frame 0 and keep >= 2 observations are reported (slot, erased bearing) for the
  // depth re-anchoring and shorter ones are dropped, without it a track is dropped when it becomes empty
  struct Shifted {
    int slot;
    double bearing[3];
  };
  void dropOldestFrame(std::vector<Shifted> *survivors);
  // feature_manager.cpp:332-351: the second newest frame is thrown away
  void dropSecondNewestFrame(int frame_count);
  void dropFailed();  // removeFailures(): solve_flag == 2

 private:
  void erase(int s);
  void compact();
  std::vector<int> id_, start_, count_, first_, flag_;
  std::vector<char> dead_;
  std::vector<double> depth_, rows_;
  std::vector<int> order_, free_;
  std::unordered_map<int, int> slot_of_;
  bool holes_ = false;
};

// InitialEXRotation (initial/initial_ex_rotation.h): the state of the online camera-IMU rotation calibration and
// CalibrationExRotation (initial_ex_rotation.cpp:13-67).  The relative camera rotation of every image (solveRelativeR) comes
// from the device (lfvio_two_view); what is left is one 4F x 4 singular value problem per image, F <= a few hundred.
struct ExRotationCalibrator {
  int frame_count = 0;
  std::vector<Matrix3d> Rc, Rimu, Rc_g;
  Matrix3d ric;
  double sv[4] = {0, 0, 0, 0};  // singular values of the last stack, falling
  ExRotationCalibrator() { clear(); }
  void clear();
  // one image: Rc = solveRelativeR's return value, delta_q = the span's pre-integrated rotation.  true (and *calib_ric) when
  // frame_count >= WINDOW_SIZE and the third-largest singular value exceeds 0.25 (:60)
  bool push(const Matrix3d &Rc_new, const Quaterniond &delta_q, Matrix3d *calib_ric);
};

// util::create_random_array(8, 0, n - 1) (initial/random_array.cc:22-49): 9 draws, sorted, made unique, cut to 8, drawn again
// until there are 8, shuffled
void drawSampleSet(std::mt19937 &rng, int n, int out[8]);

class WindowEstimator {
 public:
  WindowEstimator();
  ~WindowEstimator();
  WindowEstimator(const WindowEstimator &) = delete;

  // ---- the hot path's contract: reference names, reference semantics
  void vector2double();  // estimator.cpp:488-530
  void double2vector();  // estimator.cpp:532-600
  void optimization();   // estimator.cpp:676-1009 over include/lfvio.h
  bool collectPrior();   // waits for a marginalization still in flight (split_call) and adopts its prior; false + status on error

  // ---- relocalization (estimator.cpp:1133-1151, the branch of optimization() at :777-808, the tail of double2vector() at :603-625)
  void setReloFrame(double stamp, int index, const std::vector<Vector3d> &match_points, const Vector3d &relo_t, const Matrix3d &relo_r);
  // the reference's walk (estimator.cpp:782-806): solvable landmarks in list order with start_frame <= relo_frame_local_index, ids
  // matched in ascending order against match_points; unlike the reference the walk stops at the end of match_points.  landmark:
  // index in the window's landmark list, xy: (x, y) of the match.  Returns the number of matches.
  int reloMatches(std::vector<int> *landmark, std::vector<double> *xy) const;
  int relocalization_info = 0;
  double relo_frame_stamp = 0;
  int relo_frame_index = 0, relo_frame_local_index = 0;
  std::vector<Vector3d> match_points;
  Vector3d prev_relo_t;
  Matrix3d prev_relo_r;
  double relo_Pose[LFVIO_SIZE_POSE] = {0, 0, 0, 0, 0, 0, 1};
  Matrix3d drift_correct_r;
  Vector3d drift_correct_t;
  Vector3d relo_relative_t;
  Quaterniond relo_relative_q;
  double relo_relative_yaw = 0;
  int relo_solves = 0;  // optimization() calls that carried a relocalization message (replay statistics)

  // ---- the loop around it: processIMU / processImage / solveOdometry / slideWindow / failureDetection
  void reset();                                                     // clearState() + setParameter()
  void pushImu(double dt, const double acc[3], const double gyr[3]);
  void pushImage(double stamp, int n, const int *ids, const double *pts8);
  bool keyframeTest(int frame_count, int n, const int *ids, const double *pts8, double td);  // true: MARGIN_OLD
  void slide();
  bool diverged() const;
  void triangulate();
  void reanchorDepths(const Matrix3d &old_R, const Vector3d &old_P, const Matrix3d &new_R, const Vector3d &new_P,
                      const std::vector<TrackTable::Shifted> &tracks);
  // ESTIMATE_EXTRINSIC == 2 (estimator.cpp:142-159): the newest span's delta_q, lfvio_two_view on the matches of the two
  // newest frames, the calibrator; on success ric and the CONFIGURED ric become the calibrated one and the mode becomes 1.
  // Returns the status of the device calls.
  int calibrateExtrinsicRotation();
  ExRotationCalibrator exrot;
  struct LastTwoView {  // what the last image handed to lfvio_two_view and got back (tests, tools)
    std::vector<double> bl, br;
    std::vector<int> samples;
    std::vector<unsigned char> mask;
    LfvioTwoViewOut out;
    bool called = false;  // false: fewer than 9 matches, Rc = I without a device call
  } last_two_view;
  long long two_view_calls = 0;
  bool refreshSpans(bool all, const Vector3d *ba = nullptr, const Vector3d *bg = nullptr);  // device pre-integration of dirty spans
  void pack(LfvioWindow *w);

  // keyframe i of the window (logical index through the ring)
  Keyframe &kf(int i) { return frames_[ring_.phys(i)]; }
  const Keyframe &kf(int i) const { return frames_[ring_.phys(i)]; }
  ImuSpan &span(int i) { return spans_[ring_.phys(i)]; }
  const ImuSpan &span(int i) const { return spans_[ring_.phys(i)]; }

  enum Phase { INITIAL = 0, NON_LINEAR = 1 };
  Phase phase = INITIAL;
  int frame_count = 0;
  int marg_flag = LFVIO_MARGIN_OLD;
  bool first_imu = false, failure_occur = false, fused = true;
  Vector3d acc_prev, gyr_prev, g;  // the previous IMU sample; gravity as aligned
  Matrix3d ric, last_R, last_R0;
  Vector3d tic, last_P, last_P0;
  double td = 0, initial_timestamp = 0;
  int slides_old = 0, slides_new = 0, tracked_last = 0;
  // wall clock spent in the device-backed steps since the last reset of the timers (seconds; tools/replay_stream.py):
  // [0] optimization() up to the state, [1] collectPrior(), [2] triangulate(), [3] reanchorDepths(), [4] refreshSpans(), [5] calls of [0]
  double timers[6] = {0, 0, 0, 0, 0, 0};
  TrackTable tracks;

  struct Bootstrap {  // what initialStructure() + visualInitialAlign() would leave (estimator.cpp:222-473), from outside
    bool valid = false;
    Keyframe kf[FRAMES];
    Vector3d g;
    // optional: the depths visualInitialAlign() left (estimator.cpp:389-425: triangulated on the SfM poses, then x s), by feature
    // id.  Tracks not listed start unknown (-1) and are triangulated on the aligned state, as all of them are without this.
    std::vector<int> depth_ids;
    std::vector<double> depths;
  } bootstrap;

  // ---- initialization without a bootstrap record: visualInitialAlign() (estimator.cpp:367-443) on SfM poses from outside
  // all_image_frame (estimator.cpp:137-140): per image its stamp and the IMU samples since the previous image with the
  // constructor arguments of its IntegrationBase (tmp_pre_integration); erased as slideWindow() erases it (:1051-1067: a
  // MARGIN_OLD slide drops everything up to and including Headers[0], MARGIN_SECOND_NEW keeps the entry), cleared by reset().
  // The samples are appended as they arrive whether or not an SfM result is ever set (three push_backs per IMU sample; the
  // spans of the ring cannot be shared: MARGIN_SECOND_NEW merges two of them, the list keeps them apart).
  struct ImageFrame {
    double stamp = 0;
    std::vector<double> dt, acc, gyr;
    double acc0[3] = {0, 0, 0}, gyr0[3] = {0, 0, 0}, lin_ba[3] = {0, 0, 0}, lin_bg[3] = {0, 0, 0};
    // ImageFrame::points (estimator.cpp:134): the image's feature ids in ascending order (the iteration order of the reference's
    // std::map) and their bearings x y z as stored; kept and erased with the entry
    std::vector<int> ids;
    std::vector<double> pts;  // 3 per id
  };
  std::vector<ImageFrame> image_frames;
  // What relativePose() + GlobalSFM::construct() + the PnP loop leave in all_image_frame (estimator.cpp:250-357): per image
  // ImageFrame::R (body rotation in the SfM frame) and ImageFrame::T (camera position there, unscaled), matched to the list
  // BY STAMP.  A result that does not cover every frame of the list, or a list of more than LFVIO_MAX_IMAGE_FRAMES frames, is
  // not applied: initialization fails for that image and the window slides, as after a failed initialStructure().
  struct SfmResult {
    bool valid = false;
    std::vector<double> stamps, R, T;  // n | 9n row-major | 3n
  } sfm;
  // What GlobalSFM::construct() returns through its arguments (initial/initial_sfm.cpp:128-287; estimator.cpp:268-286): Q[i], T[i]
  // of the window's keyframes (camera rotation and position in the frame of keyframe l, unscaled) and sfm_tracked_points.  The
  // PnP loop of initialStructure() (estimator.cpp:288-357) turns it into an SfmResult: solvePnpFrames().
  struct SfmStructure {
    bool valid = false;
    std::vector<double> stamps, Q, T;  // K | 4K (w x y z) | 3K
    std::vector<int> ids;              // P, sfm_tracked_points' keys
    std::vector<double> xyz;           // 3P
  } structure;
  // estimator.cpp:288-357 on `structure`: a frame of the list whose stamp is a keyframe's takes R = Q[i] RIC^T, T = T[i]; every
  // other frame gathers (SfM point, bearing) for its features that the structure holds, in ascending id order, and ALL of them are
  // posed by ONE lfvio_pnp call; R_pnp^T RIC^T and R_pnp^T (-T_pnp) as :353-356 have them.  Fills `sfm` and returns true; false
  // (initialization fails for this image, the window slides) when the structure misses a keyframe of the window, a non-keyframe
  // has fewer than 6 correspondences (:335-340) or more than 4096, the list is longer than LFVIO_MAX_IMAGE_FRAMES, or a frame comes
  // back with status 1 (include/lfvio.h, deviation 1).  The initial guess of :308-312 is never read by the solver and is not formed.
  bool solvePnpFrames();
  struct LastPnp {  // what the last attempt passed to lfvio_pnp and got back (tests, tools)
    bool called = false;
    int rc = LFVIO_OK;
    std::vector<double> stamps;  // of the non-keyframes, in list order
    std::vector<int> offset;     // CSR over them
    std::vector<double> pw, us;
    std::vector<LfvioPnpOut> out;
  } last_pnp;
  long long pnp_calls = 0;
  // What relativePose() returns (estimator.cpp:270-277, :445-473): the rotation and unit-norm position of the newest camera in the frame
  // of camera l, and l.  Set from outside (a record wins), or by relativePose() below with Config::self_relative_pose; used by the next
  // full-window image when no bootstrap record, SfM result or SfM structure is set.
  struct RelativePose {
    bool valid = false;
    int l = 0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};  // row-major
  } relative;
  // estimator.cpp:445-473: getCorresponding(i, WINDOW_SIZE) for i = 0 .. WINDOW_SIZE - 1 as one CSR, Config::ransac_iterations sample sets
  // for every pair with more than 20 matches (ransac_rng_ / drawSampleSet, seeded as in calibrateExtrinsicRotation(); pair order, then
  // set order), ONE lfvio_relative_pose call.  Returns true with `relative` filled (l and the INTENDED output of solveRelativeRT,
  // include/lfvio.h deviation 1); false when no pair passes (the reference returns false from initialStructure() without touching
  // marginalization_flag: the window slides with the flag of the parallax test), a pair has more than 4096 matches, the return code is
  // negative or the device entry is missing (status is set then, as in constructSfm()).  There is no CPU fallback.
  bool relativePose();
  struct LastRelative {  // what the last attempt passed to lfvio_relative_pose and got back (tests, tools)
    bool called = false;
    int rc = LFVIO_OK, num_samples = 0;
    std::vector<int> offset;     // CSR over the pairs [WINDOW_SIZE + 1]
    std::vector<double> bl, br;  // [M][3]
    std::vector<int> samples;    // [WINDOW_SIZE][S][8], zeros for a pair with <= 20 matches
    LfvioRelativePoseOut out;
  } last_relative;
  long long relative_calls = 0, relative_ok = 0;  // attempts that reached lfvio_relative_pose; attempts that filled `relative`
  // estimator.cpp:250-286 on `relative`: sfm_f from the track table (every track, in f_manager.feature order, its frames start_frame ...,
  // the bearings as stored), lfvio_sfm_construct (the incremental part of GlobalSFM::construct), the triangulated points compacted into
  // lfvio_sfm_ba (its full BA, :283 applied through `accepted`), then Q, T and sfm_tracked_points (:295-314) into `structure`.  Returns
  // true with `structure` filled; false (the attempt fails and the slide is MARGIN_OLD, :284) when the chain's status is not 0,
  // accepted == 0, a return code is negative, there are no tracks or more than 4096, l is outside [0, frame_count - 1] or either device
  // entry is missing.  There is no CPU fallback.
  bool constructSfm();
  struct LastConstruct {  // what the last attempt passed to lfvio_sfm_construct / lfvio_sfm_ba and got back (tests, tools)
    bool called = false, ba_called = false;
    int rc = LFVIO_OK, ba_rc = LFVIO_OK, F = 0, l = 0;
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, T[3] = {0, 0, 0};
    std::vector<int> ids, offset, frame;  // sfm_f: feature ids [P], CSR [P + 1], observation.first [M]
    std::vector<double> bearing;          // observation.second [M][3]
    std::vector<double> c_rotation, c_translation, position;  // as lfvio_sfm_construct left them: [F][4], [F][3], [P][3]
    std::vector<int> tri_op;
    LfvioSfmConstructOut out;
    LfvioSfmBaOut ba;
  } last_construct;
  long long construct_calls = 0, construct_ok = 0;  // attempts that reached lfvio_sfm_construct; attempts that filled `structure`
  struct LastViAlign {  // what the last attempt passed to lfvio_vi_align and got back (tests, tools)
    bool called = false;
    int rc = LFVIO_OK;
    std::vector<double> stamps, R, T, x;
    std::vector<int> counts;                // samples per span, [0] = 0
    std::vector<double> head, dt, acc, gyr;  // per span linearized_ba, linearized_bg, acc_0, gyr_0 (12 doubles); the samples
    double noise[4] = {0, 0, 0, 0}, tic[3] = {0, 0, 0}, g_norm = 0;
    LfvioViAlignOut out;
  } last_vi_align;
  long long vi_align_calls = 0, vi_align_ok = 0;
  // true: the window holds the aligned state the first optimization() starts from.  The IMU-excitation check of
  // initialStructure() (estimator.cpp:224-249) only logs in the reference and is left out.
  bool visualInitialAlign();
  bool stop_after_align = false;  // tests: advanceWindow() returns behind a successful alignment, before the first optimization()

  // the flat parameter arrays Ceres sees (estimator.h:107-113)
  double para_Pose[FRAMES][LFVIO_SIZE_POSE];
  double para_SpeedBias[FRAMES][LFVIO_SIZE_SPEEDBIAS];
  double para_Ex_Pose[1][LFVIO_SIZE_POSE];
  double para_Td[1][1];
  std::vector<double> para_Feature;

  bool has_prior = false;
  LfvioPrior prior;  // last_marginalization_info + its parameter blocks, (kind, frame)-tagged
  LfvioSolution summary;
  int status = LFVIO_OK;
  lfvio_ctx *gpu = nullptr;      // the context (of the first device of the mask): triangulation, depth shifts, preintegration
  lfvio_group *group = nullptr;  // more than one device in Config::device_mask: the sharded optimization()
  bool device();  // creates `gpu` (and `group`) at the first use; false, with `status` set, where there is no device

 private:
  LfvioPrior next_;  // the prior being downloaded (240 KB: a member, not a stack object; only header + n x n + n are copied)
  bool chain_upload_ = false;   // pack() on behalf of an optimization() whose upload collects the pending prior itself
  bool prior_pending_ = false;  // the marginalization of the last optimization() has not been collected yet (collectPrior)
  bool prior_on_device_ = false;  // the resident window took its prior over on the device (lfvio_batch_upload_chained_device): `prior` is stale
  bool applyBootstrap();
  ImageFrame pending_;  // tmp_pre_integration: the samples since the last image
  void advanceWindow(double stamp);  // processImage() behind the keyframe test and the calibration (estimator.cpp:161-220)
  std::mt19937 ransac_rng_;
  void seedRansac();  // on first use and whenever Config::ransac_seed changed
  bool ransac_seeded_ = false;
  unsigned ransac_seed_used_ = 0;
  void optimizationRelo();  // optimization() with relocalization_info set: lfvio_solve_relo, double2vector(), lfvio_marginalize
  std::vector<int> relo_lm_;
  std::vector<double> relo_xy_;
  FrameRing ring_;
  Keyframe frames_[FRAMES];
  ImuSpan spans_[FRAMES];
  struct Staging {  // backing store of the pointers in LfvioWindow; grows, never shrinks
    std::vector<int> start_frame, obs_offset;
    std::vector<double> inv_depth, point, velocity, cur_td, uv_y, lam_out;
  } stage_;
};

}  // namespace lfvio
