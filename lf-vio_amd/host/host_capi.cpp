// host_capi.cpp — extern "C" driver of the host side (window_estimator.h), so that the Python tests and tools can
// exercise it the way estimator_node.cpp drives the reference's Estimator.  Frames are addressed by their LOGICAL
// index 0..10 (oldest..newest); the ring underneath is not visible here.
#include <algorithm>
#include <cstring>

#include "replay.h"
#include "window_estimator.h"

using namespace lfvio;

namespace {
inline WindowEstimator *E(void *h) { return (WindowEstimator *)h; }
inline Vector3d v3(const double *a) { return Vector3d(a[0], a[1], a[2]); }
inline void setM(Matrix3d &m, const double *a) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m(i, j) = a[i * 3 + j];
}
inline void getM(const Matrix3d &m, double *a) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) a[i * 3 + j] = m(i, j);
}
}  // namespace

extern "C" {

void *lfvio_host_create(void) { return new WindowEstimator(); }
void lfvio_host_destroy(void *h) { delete E(h); }

// the YAML / parameters.cpp values; p = {ACC_N, GYR_N, ACC_W, GYR_W, g_norm, TR, ROW, SOLVER_TIME, TD}
void lfvio_host_set_params(const double *p, int estimate_extrinsic, int estimate_td, int num_iterations) {
  Config &c = config();
  c.acc_n = p[0], c.gyr_n = p[1], c.acc_w = p[2], c.gyr_w = p[3];
  c.gravity[0] = 0, c.gravity[1] = 0, c.gravity[2] = p[4];
  c.tr = p[5], c.row = p[6], c.solver_time = p[7], c.td = p[8];
  c.estimate_extrinsic = estimate_extrinsic, c.estimate_td = estimate_td, c.num_iterations = num_iterations;
}
// the configured extrinsic (TIC / RIC of the YAML file): what a reset restores
void lfvio_host_set_extrinsic(const double *tic, const double *ric) {
  std::memcpy(config().tic, tic, sizeof config().tic);
  std::memcpy(config().ric, ric, sizeof config().ric);
}
// the configured time offset (TD of the YAML file) on its own: what a reset restores.  A recording whose initialization comes from
// SfM records carries no extrinsic or td (a bootstrap record does): they are configured, as in the node
void lfvio_host_set_td(double td) { config().td = td; }
// SOLVER_TIME on its own (<= 0: no wall-clock cap — what a test on a loaded machine wants: Ceres' max_solver_time_in_seconds makes the
// number of iterations depend on the clock)
void lfvio_host_set_solver_time(double seconds) { config().solver_time = seconds; }
void lfvio_host_set_min_parallax(double keyframe_parallax_px) { config().min_parallax = keyframe_parallax_px / FOCAL_LENGTH; }

void lfvio_host_set_state(void *h, const double *Ps, const double *Rs, const double *Vs, const double *Bas, const double *Bgs,
                          const double *tic, const double *ric, double td) {
  WindowEstimator *e = E(h);
  for (int i = 0; i < FRAMES; i++) {
    Keyframe &f = e->kf(i);
    f.P = v3(Ps + 3 * i), f.V = v3(Vs + 3 * i), f.Ba = v3(Bas + 3 * i), f.Bg = v3(Bgs + 3 * i);
    setM(f.R, Rs + 9 * i);
  }
  e->tic = v3(tic);
  setM(e->ric, ric);
  e->td = td;
}

void lfvio_host_get_state(void *h, double *Ps, double *Rs, double *Vs, double *Bas, double *Bgs, double *tic, double *ric, double *td) {
  WindowEstimator *e = E(h);
  for (int i = 0; i < FRAMES; i++) {
    const Keyframe &f = e->kf(i);
    for (int k = 0; k < 3; k++) Ps[3 * i + k] = f.P(k), Vs[3 * i + k] = f.V(k), Bas[3 * i + k] = f.Ba(k), Bgs[3 * i + k] = f.Bg(k);
    getM(f.R, Rs + 9 * i);
  }
  for (int k = 0; k < 3; k++) tic[k] = e->tic(k);
  getM(e->ric, ric);
  *td = e->td;
}

void lfvio_host_clear_features(void *h) { E(h)->tracks.clear(); }

// a whole track: obs n x 8 = [bearing xyz, pixel uv, bearing-velocity xyz] like the 8-vector of estimator_node.cpp:308
void lfvio_host_add_feature(void *h, int id, int start_frame, int n, const double *obs, const double *cur_td, double estimated_depth) {
  TrackTable &t = E(h)->tracks;
  const int s = t.create(id, start_frame);
  for (int k = 0; k < n; k++) t.append(s, obs + 8 * k, cur_td[k]);
  t.setDepth(s, estimated_depth);
}

int lfvio_host_triangulate(void *h) {
  WindowEstimator *e = E(h);
  e->status = LFVIO_OK;
  e->triangulate();
  return e->status;
}
// the depth re-anchoring of a MARGIN_OLD slide with the marginalized frame's pose given (back_R0, back_P0) and the
// estimator's frame 0 as the new anchor frame (estimator.cpp:1120-1127)
int lfvio_host_remove_back_shift_depth(void *h, const double *back_R0, const double *back_P0) {
  WindowEstimator *e = E(h);
  Matrix3d bR;
  setM(bR, back_R0);
  const Vector3d bP = v3(back_P0);
  e->status = LFVIO_OK;
  std::vector<TrackTable::Shifted> moved;
  e->tracks.dropOldestFrame(&moved);
  e->reanchorDepths(bR * e->ric, bP + bR * e->tic, e->kf(0).R * e->ric, e->kf(0).P + e->kf(0).R * e->tic, moved);
  return e->status;
}
void lfvio_host_set_depths(void *h, const double *d, int n) {
  TrackTable &t = E(h)->tracks;
  int k = 0;
  for (int s : t.order())
    if (k < n) t.setDepth(s, d[k++]);
}
int lfvio_host_num_features(void *h) { return E(h)->tracks.live(); }
// (feature_id, start_frame, number of observations, estimated_depth) of every track in table order
void lfvio_host_list_features(void *h, int *ids, int *start, int *count, double *depth) {
  const TrackTable &t = E(h)->tracks;
  int k = 0;
  for (int s : t.order()) ids[k] = t.id(s), start[k] = t.start(s), count[k] = t.count(s), depth[k] = t.depth(s), k++;
}
int lfvio_host_feature_count(void *h) { return E(h)->tracks.solvableCount(); }
void lfvio_host_get_depths(void *h, double *out) {
  const TrackTable &t = E(h)->tracks;
  int k = 0;
  for (int s : t.order()) out[k++] = t.depth(s);
}

// span `frame` (the samples between keyframes frame - 1 and frame) := {acc0, gyr0, ba, bg} + n samples
void lfvio_host_set_imu(void *h, int frame, const double *acc0, const double *gyr0, const double *ba, const double *bg, int n,
                        const double *dt, const double *acc, const double *gyr) {
  ImuSpan &sp = E(h)->span(frame);
  sp.open(v3(acc0), v3(gyr0), v3(ba), v3(bg));
  for (int k = 0; k < n; k++) sp.push(dt[k], acc + 3 * k, gyr + 3 * k);
}

void lfvio_host_repropagate(void *h, int frame, const double *ba, const double *bg) {
  ImuSpan &sp = E(h)->span(frame);
  if (!sp.present) return;
  std::memcpy(sp.lin_ba, ba, sizeof sp.lin_ba), std::memcpy(sp.lin_bg, bg, sizeof sp.lin_bg);
  sp.dirty = true;
}

// ba, bg: [11][3]; every present span is integrated again in one device call; returns the status
int lfvio_host_repropagate_window(void *h, const double *ba, const double *bg) {
  WindowEstimator *e = E(h);
  Vector3d a[FRAMES], g[FRAMES];
  for (int i = 0; i < FRAMES; i++) a[i] = v3(ba + 3 * i), g[i] = v3(bg + 3 * i);
  e->status = LFVIO_OK;
  e->refreshSpans(true, a, g);
  return e->status;
}

void lfvio_host_process_imu(void *h, double dt, const double *acc, const double *gyr) { E(h)->pushImu(dt, acc, gyr); }

// ids[n], pts[n][8] = x y z u v vx vy vz (camera 0); returns the status of the device calls inside
int lfvio_host_process_image(void *h, double stamp, int n, const int *ids, const double *pts) {
  WindowEstimator *e = E(h);
  e->status = LFVIO_OK;
  e->pushImage(stamp, n, ids, pts);
  return e->status;
}

// only the keyframe decision of an image: appends the observations, returns 1 for MARGIN_OLD
int lfvio_host_add_feature_check_parallax(void *h, int frame_count, int n, const int *ids, const double *pts, double td) {
  return E(h)->keyframeTest(frame_count, n, ids, pts, td) ? 1 : 0;
}

// Ps Rs Vs Bas Bgs as lfvio_host_set_state, g[3]
void lfvio_host_set_bootstrap(void *h, const double *Ps, const double *Rs, const double *Vs, const double *Bas, const double *Bgs, const double *g) {
  WindowEstimator::Bootstrap &b = E(h)->bootstrap;
  for (int i = 0; i < FRAMES; i++) {
    b.kf[i].P = v3(Ps + 3 * i), b.kf[i].V = v3(Vs + 3 * i), b.kf[i].Ba = v3(Bas + 3 * i), b.kf[i].Bg = v3(Bgs + 3 * i);
    setM(b.kf[i].R, Rs + 9 * i);
  }
  b.g = v3(g);
  b.depth_ids.clear(), b.depths.clear();  // a state set without depths has none (lfvio_host_set_bootstrap_depths comes after this call)
  b.valid = true;
}

// optional, after lfvio_host_set_bootstrap: the depths that belong to that state, by feature id (Bootstrap::depths)
void lfvio_host_set_bootstrap_depths(void *h, int n, const int *ids, const double *depths) {
  WindowEstimator::Bootstrap &b = E(h)->bootstrap;
  b.depth_ids.assign(ids, ids + n), b.depths.assign(depths, depths + n);
}

// the window is already filled from outside (set_state / add_feature / set_imu): continue in the running phase
void lfvio_host_set_running(void *h, const double *stamps, const double *acc_0, const double *gyr_0, const double *g) {
  WindowEstimator *e = E(h);
  e->phase = WindowEstimator::NON_LINEAR;
  e->frame_count = WINDOW_SIZE;
  e->first_imu = true;
  for (int i = 0; i < FRAMES; i++) e->kf(i).stamp = stamps[i];
  e->acc_prev = v3(acc_0), e->gyr_prev = v3(gyr_0), e->g = v3(g);
  e->last_R = e->kf(WINDOW_SIZE).R, e->last_P = e->kf(WINDOW_SIZE).P, e->last_R0 = e->kf(0).R, e->last_P0 = e->kf(0).P;
}

void lfvio_host_clear_state(void *h) { E(h)->reset(); }
void lfvio_host_slide_window(void *h) { E(h)->slide(); }
int lfvio_host_failure_detection(void *h) { return E(h)->diverged() ? 1 : 0; }

// out = {phase, marginalization flag, frame_count, old-frame slides, second-new slides, tracks continued by the last image, tracks, failure_occur}
void lfvio_host_get_flow(void *h, int *out) {
  WindowEstimator *e = E(h);
  out[0] = e->phase, out[1] = e->marg_flag, out[2] = e->frame_count, out[3] = e->slides_old, out[4] = e->slides_new;
  out[5] = e->tracked_last, out[6] = e->tracks.live(), out[7] = e->failure_occur ? 1 : 0;
}

// per frame: stamp, number of buffered IMU samples, span present, its sum_dt
void lfvio_host_get_buffers(void *h, double *stamps, int *num_samples, int *has_pre, double *sum_dt) {
  WindowEstimator *e = E(h);
  for (int i = 0; i < FRAMES; i++) {
    const ImuSpan &sp = e->span(i);
    stamps[i] = e->kf(i).stamp, num_samples[i] = sp.samples(), has_pre[i] = sp.present ? 1 : 0, sum_dt[i] = sp.present ? sp.sum_dt : 0.0;
  }
}

// Replays an LFVT trace (replay.h) and writes the trajectory file.
// stats (may be null) = {images, thrown, keyframes, non_keyframes, poses, failures, last_status, iterations, restarts, bootstraps}
int lfvio_host_replay(void *h, const char *trace_path, const char *traj_path, int max_images, int *stats) {
  Trace trace;
  if (!trace.load(trace_path)) return -3;
  ReplayStats st;
  int rc = replay(*E(h), trace, traj_path, max_images, &st);
  if (stats) std::memcpy(stats, &st, sizeof st);
  return rc;
}

// the same with the wall-clock milliseconds of every image handed over (ms[cap]); *n_ms = how many were written
int lfvio_host_replay_timed(void *h, const char *trace_path, const char *traj_path, int max_images, int *stats, double *ms, int cap, int *n_ms) {
  Trace trace;
  if (!trace.load(trace_path)) return -3;
  ReplayStats st;
  std::vector<double> t;
  int rc = replay(*E(h), trace, traj_path, max_images, &st, &t);
  if (stats) std::memcpy(stats, &st, sizeof st);
  const int n = std::min((int)t.size(), cap);
  if (ms) std::memcpy(ms, t.data(), sizeof(double) * n);
  if (n_ms) *n_ms = n;
  return rc;
}

// the decode of one feature record, for the wire-format test: fills ids[n] (ascending), pts[n][8]; returns n
int lfvio_host_decode_features(const char *trace_path, int image_index, int cap, int *ids, double *pts, double *stamp) {
  Trace trace;
  if (!trace.load(trace_path) || image_index < 0 || image_index >= (int)trace.images.size()) return -1;
  DecodedImage img;
  decodeFeatures(trace.images[image_index], &img);
  *stamp = trace.images[image_index].t;
  const int n = std::min((int)img.ids.size(), cap);
  std::memcpy(ids, img.ids.data(), sizeof(int) * n);
  std::memcpy(pts, img.pts.data(), sizeof(double) * 8 * n);
  return n;
}

void lfvio_host_vector2double(void *h) { E(h)->vector2double(); }
void lfvio_host_double2vector(void *h) { E(h)->double2vector(); }

void lfvio_host_get_para(void *h, double *pose, double *sb, double *ex, double *td, double *feature) {
  WindowEstimator *e = E(h);
  std::memcpy(pose, e->para_Pose, sizeof e->para_Pose);
  std::memcpy(sb, e->para_SpeedBias, sizeof e->para_SpeedBias);
  std::memcpy(ex, e->para_Ex_Pose[0], sizeof e->para_Ex_Pose[0]);
  *td = e->para_Td[0][0];
  std::copy(e->para_Feature.begin(), e->para_Feature.end(), feature);
}
void lfvio_host_set_para(void *h, const double *pose, const double *sb, const double *ex, double td, const double *feature, int n) {
  WindowEstimator *e = E(h);
  std::memcpy(e->para_Pose, pose, sizeof e->para_Pose);
  std::memcpy(e->para_SpeedBias, sb, sizeof e->para_SpeedBias);
  std::memcpy(e->para_Ex_Pose[0], ex, sizeof e->para_Ex_Pose[0]);
  e->para_Td[0][0] = td;
  e->para_Feature.assign(feature, feature + n);
}

// LfvioWindow exactly as optimization() hands it to the C-ABI (pointers stay valid until the next pack); returns the
// status of the device pre-integration of the spans that needed it
int lfvio_host_pack(void *h, LfvioWindow *out) {
  WindowEstimator *e = E(h);
  e->status = LFVIO_OK;
  e->refreshSpans(false);
  e->vector2double();
  e->pack(out);
  return e->status;
}

void lfvio_host_set_flag(void *h, int flag) { E(h)->marg_flag = flag; }
void lfvio_host_set_prior(void *h, const LfvioPrior *p) {
  WindowEstimator *e = E(h);
  (void)e->collectPrior();
  e->has_prior = p && p->valid;
  if (e->has_prior) e->prior = *p;
}
int lfvio_host_get_prior(void *h, LfvioPrior *out) {
  WindowEstimator *e = E(h);
  (void)e->collectPrior();
  if (!e->has_prior) {
    out->valid = 0;
    return 0;
  }
  *out = e->prior;
  return 1;
}

// 1 (default): one upload, everything on the device; 0: the literal lfvio_solve / double2vector / lfvio_marginalize flow
void lfvio_host_set_fused(void *h, int on) { E(h)->fused = on != 0; }
// HIP devices of the estimator (bit d = device d); before the first call that needs the device.  More than one bit: the
// optimization() of every frame runs landmark-sharded through an lfvio_group over them.
void lfvio_host_set_device_mask(unsigned mask) { config().device_mask = mask ? mask : 1u; }
void lfvio_host_set_local_shards(int n) { config().local_shards = n; }
void lfvio_host_set_split_call(int on) { config().split_call = on != 0; }
void lfvio_host_set_device_chain(int on) { config().device_chain = on != 0; }

// Estimator::setReloFrame (estimator.cpp:1133-1151): pts n x (x, y, id), relo_r row-major
void lfvio_host_set_relo_frame(void *h, double stamp, int index, int n, const double *pts, const double *relo_t, const double *relo_r) {
  std::vector<Vector3d> mp;
  for (int k = 0; k < n; k++) mp.push_back(v3(pts + 3 * k));
  Matrix3d R;
  setM(R, relo_r);
  E(h)->setReloFrame(stamp, index, mp, v3(relo_t), R);
}
// the relocalization members: out[30] = relocalization_info, relo_frame_local_index, relo_Pose[7], drift_correct_r[9] (row-major),
// drift_correct_t[3], relo_relative_t[3], relo_relative_q[4] (x y z w), relo_relative_yaw, relo_solves
void lfvio_host_get_relo(void *h, double *out) {
  WindowEstimator *e = E(h);
  out[0] = e->relocalization_info, out[1] = e->relo_frame_local_index;
  for (int k = 0; k < 7; k++) out[2 + k] = e->relo_Pose[k];
  getM(e->drift_correct_r, out + 9);
  for (int k = 0; k < 3; k++) out[18 + k] = e->drift_correct_t(k), out[21 + k] = e->relo_relative_t(k);
  out[24] = e->relo_relative_q.x(), out[25] = e->relo_relative_q.y(), out[26] = e->relo_relative_q.z(), out[27] = e->relo_relative_q.w();
  out[28] = e->relo_relative_yaw, out[29] = e->relo_solves;
}
// the match list optimization() would build now: landmark[cap], xy[cap][2]; returns K (at most cap written)
int lfvio_host_relo_matches(void *h, int cap, int *landmark, double *xy) {
  std::vector<int> l;
  std::vector<double> p;
  const int K = E(h)->reloMatches(&l, &p);
  for (int k = 0; k < K && k < cap; k++) landmark[k] = l[k], xy[2 * k] = p[2 * k], xy[2 * k + 1] = p[2 * k + 1];
  return K;
}
// waits for the marginalization a split optimization() left running and adopts its prior (what the next pack() would do)
int lfvio_host_collect_prior(void *h) { return E(h)->collectPrior() ? 0 : E(h)->status; }
void lfvio_host_get_timers(void *h, double *out6, int reset) {
  WindowEstimator *e = E(h);
  for (int k = 0; k < 6; k++) {
    out6[k] = e->timers[k];
    if (reset) e->timers[k] = 0.0;
  }
}
int lfvio_host_uses_group(void *h) { return E(h)->group != nullptr; }

// ---- ESTIMATE_EXTRINSIC == 2: the online camera-IMU rotation calibration
// RANSAC settings of the two-view step (process-wide, like the other parameters); seed 0 = std::random_device
void lfvio_host_set_ransac(unsigned seed, int iterations) { config().ransac_seed = seed, config().ransac_iterations = iterations; }
// the process-wide mode and configured extrinsic as they are NOW (a successful calibration rewrites both)
int lfvio_host_get_estimate_extrinsic(void) { return config().estimate_extrinsic; }
void lfvio_host_set_estimate_extrinsic(int mode) { config().estimate_extrinsic = mode; }
void lfvio_host_get_extrinsic(double *tic, double *ric) {
  std::memcpy(tic, config().tic, sizeof config().tic);
  std::memcpy(ric, config().ric, sizeof config().ric);
}
// CalibrationExRotation alone, no device: Rc row-major, delta_q = (x, y, z, w); ric_out[9], sv_out[4]; returns 1 on success
int lfvio_host_exrot_push(void *h, const double *Rc, const double *delta_q, double *ric_out, double *sv_out) {
  ExRotationCalibrator &x = E(h)->exrot;
  Matrix3d R, calib;
  setM(R, Rc);
  const bool ok = x.push(R, Quaterniond(delta_q[3], delta_q[0], delta_q[1], delta_q[2]), &calib);
  getM(x.ric, ric_out);
  std::memcpy(sv_out, x.sv, sizeof x.sv);
  return ok ? 1 : 0;
}
// frame_count of the calibrator; its ric and last singular values
int lfvio_host_exrot_state(void *h, double *ric_out, double *sv_out) {
  const ExRotationCalibrator &x = E(h)->exrot;
  getM(x.ric, ric_out);
  std::memcpy(sv_out, x.sv, sizeof x.sv);
  return x.frame_count;
}
void lfvio_host_exrot_clear(void *h) { E(h)->exrot.clear(); }
// the pair the last push added: Rc (solveRelativeR's return value) and Rimu (delta_q as a matrix), row-major
void lfvio_host_exrot_last(void *h, double *Rc, double *Rimu) {
  const ExRotationCalibrator &x = E(h)->exrot;
  getM(x.Rc.back(), Rc), getM(x.Rimu.back(), Rimu);
}
// What the last image of mode 2 handed to lfvio_two_view: counts[2] = {matches, sample sets (0: fewer than 9 matches, no device
// call)}; the arrays (any may be null) take at most cap_matches matches / cap_samples sets.  Returns the number of device calls so far.
long long lfvio_host_last_two_view(void *h, int cap_matches, int cap_samples, int *counts, double *bl, double *br, int *samples,
                                   unsigned char *mask, LfvioTwoViewOut *out) {
  const WindowEstimator::LastTwoView &t = E(h)->last_two_view;
  const int N = (int)t.bl.size() / 3, S = t.called ? (int)t.samples.size() / 8 : 0;
  counts[0] = N, counts[1] = S;
  const size_t n = (size_t)std::min(N, cap_matches), s = (size_t)std::min(S, cap_samples);
  if (bl && n) std::memcpy(bl, t.bl.data(), n * 24);
  if (br && n) std::memcpy(br, t.br.data(), n * 24);
  if (samples && s) std::memcpy(samples, t.samples.data(), s * 32);
  if (mask && n && t.called) std::memcpy(mask, t.mask.data(), n);
  if (out && t.called) *out = t.out;
  return E(h)->two_view_calls;
}
long long lfvio_host_two_view_calls(void *h) { return E(h)->two_view_calls; }
// getCorresponding(l, r): bl, br [cap][3]; returns the number of matches
int lfvio_host_corresponding(void *h, int l, int r, int cap, double *bl, double *br) {
  std::vector<double> a, b;
  const int n = E(h)->tracks.corresponding(l, r, &a, &b);
  const size_t k = (size_t)std::min(n, cap);
  if (k) std::memcpy(bl, a.data(), k * 24), std::memcpy(br, b.data(), k * 24);
  return n;
}
// util::create_random_array(8, 0, n - 1), `count` sets from a generator seeded with `seed`
void lfvio_host_draw_samples(unsigned seed, int n, int count, int *out) {
  std::mt19937 rng(seed);
  for (int k = 0; k < count; k++) drawSampleSet(rng, n, out + 8 * k);
}

// ---- initialization from SfM poses (WindowEstimator::visualInitialAlign)
// SfmResult: n frames, stamps[n], R[n][9] row-major (ImageFrame::R), T[n][3] (ImageFrame::T); used by the next full-window image
void lfvio_host_set_sfm(void *h, int n, const double *stamps, const double *R, const double *T) {
  WindowEstimator::SfmResult &s = E(h)->sfm;
  s.stamps.assign(stamps, stamps + n), s.R.assign(R, R + 9 * (size_t)n), s.T.assign(T, T + 3 * (size_t)n);
  s.valid = true;
}
// SfmStructure (what GlobalSFM::construct() returns): K keyframes stamps[K], Q[K][4] (w x y z), T[K][3]; P points ids[P], xyz[P][3];
// used by the next full-window image when neither a bootstrap record nor an SfM result is set
void lfvio_host_set_sfm_structure(void *h, int K, const double *stamps, const double *Q, const double *T, int P, const int *ids, const double *xyz) {
  WindowEstimator::SfmStructure &s = E(h)->structure;
  s.stamps.assign(stamps, stamps + K), s.Q.assign(Q, Q + 4 * (size_t)K), s.T.assign(T, T + 3 * (size_t)K);
  s.ids.assign(ids, ids + P), s.xyz.assign(xyz, xyz + 3 * (size_t)P);
  s.valid = true;
}
// RelativePose (what relativePose() returns): l, R[9] row-major, T[3]; used by the next full-window image when no bootstrap record, SfM
// result or SfM structure is set: the estimator runs GlobalSFM::construct() on the device (WindowEstimator::constructSfm), then the PnP
// loop and the alignment
void lfvio_host_set_relative_pose(void *h, int l, const double *R, const double *T) {
  WindowEstimator::RelativePose &r = E(h)->relative;
  r.l = l;
  std::memcpy(r.R, R, sizeof r.R), std::memcpy(r.T, T, sizeof r.T);
  r.valid = true;
}
// the SfM structure as the estimator holds it (after constructSfm(), or as set): counts[2] = {K, P}; any array may be null and takes at
// most cap_kf / cap_pts entries: stamps[K], Q[K][4], T[K][3], ids[P], xyz[P][3]
void lfvio_host_get_sfm_structure(void *h, int cap_kf, int cap_pts, int *counts, double *stamps, double *Q, double *T, int *ids, double *xyz) {
  const WindowEstimator::SfmStructure &s = E(h)->structure;
  counts[0] = (int)s.stamps.size(), counts[1] = (int)s.ids.size();
  const size_t k = std::min(s.stamps.size(), (size_t)std::max(cap_kf, 0)), p = std::min(s.ids.size(), (size_t)std::max(cap_pts, 0));
  if (stamps && k) std::memcpy(stamps, s.stamps.data(), k * 8);
  if (Q && k && s.Q.size() >= 4 * k) std::memcpy(Q, s.Q.data(), k * 32);
  if (T && k && s.T.size() >= 3 * k) std::memcpy(T, s.T.data(), k * 24);
  if (ids && p) std::memcpy(ids, s.ids.data(), p * 4);
  if (xyz && p && s.xyz.size() >= 3 * p) std::memcpy(xyz, s.xyz.data(), p * 24);
}
// What the last attempt handed to lfvio_sfm_construct / lfvio_sfm_ba and got back.  info[8] = {frames F, l, points P, observations M,
// construct call made, its return code, BA call made, its return code}; the arrays (any may be null) take at most cap_points points /
// cap_obs observations: ids[P], offset[P + 1], frame[M], bearing[M][3], rel[12] = relative_R, relative_T, and as lfvio_sfm_construct left
// them c_rotation[F][4], c_translation[F][3], position[P][3], tri_op[P]; out, ba.  Returns the number of lfvio_sfm_construct calls so far.
long long lfvio_host_last_construct(void *h, int cap_points, int cap_obs, int *info, int *ids, int *offset, int *frame, double *bearing, double *rel,
                                    double *c_rotation, double *c_translation, double *position, int *tri_op, LfvioSfmConstructOut *out, LfvioSfmBaOut *ba) {
  const WindowEstimator::LastConstruct &v = E(h)->last_construct;
  const int P = (int)v.ids.size(), M = (int)v.frame.size();
  info[0] = v.F, info[1] = v.l, info[2] = P, info[3] = M, info[4] = v.called ? 1 : 0, info[5] = v.rc, info[6] = v.ba_called ? 1 : 0, info[7] = v.ba_rc;
  const bool fits = P <= cap_points && M <= cap_obs;
  if (fits && P) {
    if (ids) std::memcpy(ids, v.ids.data(), (size_t)P * 4);
    if (offset) std::memcpy(offset, v.offset.data(), ((size_t)P + 1) * 4);
    if (frame && M) std::memcpy(frame, v.frame.data(), (size_t)M * 4);
    if (bearing && M) std::memcpy(bearing, v.bearing.data(), (size_t)M * 24);
    if (position && v.position.size() == 3 * (size_t)P) std::memcpy(position, v.position.data(), (size_t)P * 24);
    if (tri_op && v.tri_op.size() == (size_t)P) std::memcpy(tri_op, v.tri_op.data(), (size_t)P * 4);
  }
  if (rel) std::memcpy(rel, v.R, 72), std::memcpy(rel + 9, v.T, 24);
  if (c_rotation && !v.c_rotation.empty()) std::memcpy(c_rotation, v.c_rotation.data(), v.c_rotation.size() * 8);
  if (c_translation && !v.c_translation.empty()) std::memcpy(c_translation, v.c_translation.data(), v.c_translation.size() * 8);
  if (out) *out = v.out;
  if (ba) *ba = v.ba;
  return E(h)->construct_calls;
}
// out[2] = {attempts that reached lfvio_sfm_construct, attempts that filled the SfM structure}
void lfvio_host_construct_counts(void *h, long long *out) { out[0] = E(h)->construct_calls, out[1] = E(h)->construct_ok; }
// Config::self_relative_pose: a full-window image without any record runs relativePose() on the device (process-wide, like the mode)
void lfvio_host_set_self_relative_pose(int on) { config().self_relative_pose = on != 0; }
// What the last attempt handed to lfvio_relative_pose and got back.  info[4] = {matches M, sample sets per pair S, call made, its return
// code}; the arrays (any may be null) take at most cap_matches matches / cap_samples sets per pair: offset[WINDOW_SIZE + 1], bl[M][3],
// br[M][3], samples[WINDOW_SIZE][S][8]; out.  Returns the number of lfvio_relative_pose calls so far.
long long lfvio_host_last_relative(void *h, int cap_matches, int cap_samples, int *info, int *offset, double *bl, double *br, int *samples,
                                   LfvioRelativePoseOut *out) {
  const WindowEstimator::LastRelative &v = E(h)->last_relative;
  const int M = v.offset.empty() ? 0 : v.offset.back(), S = v.num_samples;
  info[0] = M, info[1] = S, info[2] = v.called ? 1 : 0, info[3] = v.rc;
  if (offset)
    for (size_t k = 0; k < v.offset.size() && k <= (size_t)WINDOW_SIZE; k++) offset[k] = v.offset[k];
  if (M <= cap_matches) {
    if (bl) std::memcpy(bl, v.bl.data(), v.bl.size() * sizeof(double));
    if (br) std::memcpy(br, v.br.data(), v.br.size() * sizeof(double));
  }
  if (samples && S <= cap_samples) std::memcpy(samples, v.samples.data(), v.samples.size() * sizeof(int));
  if (out) *out = v.out;
  return E(h)->relative_calls;
}
// out[2] = {attempts that reached lfvio_relative_pose, attempts that filled the relative pose}
void lfvio_host_relative_counts(void *h, long long *out) { out[0] = E(h)->relative_calls, out[1] = E(h)->relative_ok; }
// the sample sets relativePose() draws from std::mt19937(seed) for pairs of n[0 .. pairs) matches: `count` sets per pair with n > 20, pair
// order, then set order; out[pairs][count][8], zeros for the other pairs
void lfvio_host_draw_pair_samples(unsigned seed, int pairs, const int *n, int count, int *out) {
  std::mt19937 rng(seed);
  std::memset(out, 0, (size_t)pairs * count * 8 * sizeof(int));
  for (int p = 0; p < pairs; p++)
    if (n[p] > 20)
      for (int k = 0; k < count; k++) drawSampleSet(rng, n[p], out + ((size_t)p * count + k) * 8);
}
// ImageFrame::points of entry k of all_image_frame: ids[cap], pts[cap][3]; returns their number, -1: no such entry
int lfvio_host_image_frame_points(void *h, int k, int cap, int *ids, double *pts) {
  const std::vector<WindowEstimator::ImageFrame> &l = E(h)->image_frames;
  if (k < 0 || k >= (int)l.size()) return -1;
  const size_t n = std::min(l[k].ids.size(), (size_t)std::max(cap, 0));
  if (n && ids) std::memcpy(ids, l[k].ids.data(), n * 4);
  if (n && pts) std::memcpy(pts, l[k].pts.data(), n * 24);
  return (int)l[k].ids.size();
}
// What the last attempt handed to lfvio_pnp and got back.  info[4] = {non-keyframes F, correspondences M, device call made, its
// return code}; the arrays (any may be null) take at most cap_frames / cap_points: stamps[F], offset[F + 1], pw[M][3], us[M][3],
// out[F].  Returns the number of device calls so far.
long long lfvio_host_last_pnp(void *h, int cap_frames, int cap_points, int *info, double *stamps, int *offset, double *pw, double *us, LfvioPnpOut *out) {
  const WindowEstimator::LastPnp &v = E(h)->last_pnp;
  const int F = (int)v.stamps.size(), M = (int)(v.us.size() / 3);
  info[0] = F, info[1] = M, info[2] = v.called ? 1 : 0, info[3] = v.rc;
  const size_t f = (size_t)std::min(F, cap_frames), m = (size_t)std::min(M, cap_points);
  if (stamps && f) std::memcpy(stamps, v.stamps.data(), f * 8);
  if (offset && f && f == (size_t)F) std::memcpy(offset, v.offset.data(), (f + 1) * 4);
  if (pw && m) std::memcpy(pw, v.pw.data(), m * 24);
  if (us && m) std::memcpy(us, v.us.data(), m * 24);
  if (out && f && v.out.size() >= f) std::memcpy(out, v.out.data(), f * sizeof(LfvioPnpOut));
  return E(h)->pnp_calls;
}
// the SfM result as the estimator holds it (after solvePnpFrames(): every frame of the list): returns n; stamps[cap], R[cap][9], T[cap][3]
int lfvio_host_get_sfm(void *h, int cap, double *stamps, double *R, double *T) {
  const WindowEstimator::SfmResult &s = E(h)->sfm;
  const size_t n = std::min(s.stamps.size(), (size_t)std::max(cap, 0));
  if (n) std::memcpy(stamps, s.stamps.data(), n * 8), std::memcpy(R, s.R.data(), n * 72), std::memcpy(T, s.T.data(), n * 24);
  return (int)s.stamps.size();
}
// all_image_frame: stamps[cap], samples per entry [cap]; returns the length of the list
int lfvio_host_image_frames(void *h, int cap, double *stamps, int *num_samples) {
  const std::vector<WindowEstimator::ImageFrame> &l = E(h)->image_frames;
  for (int k = 0; k < (int)l.size() && k < cap; k++) stamps[k] = l[k].stamp, num_samples[k] = (int)l[k].dt.size();
  return (int)l.size();
}
// What the last attempt handed to lfvio_vi_align and got back.  info[4] = {frames F, samples in all spans, device call made, its
// return code}; the arrays (any may be null) take at most cap_frames frames / cap_samples samples: stamps[F], R[F][9], T[F][3],
// counts[F], head[F][12] (linearized_ba, linearized_bg, acc_0, gyr_0 per span), dt / acc / gyr of all spans in order,
// params[8] = noise[4], tic[3], g_norm; out and x[3F] as the call left them.  Returns the number of device calls so far.
long long lfvio_host_last_vi_align(void *h, int cap_frames, int cap_samples, int *info, double *stamps, double *R, double *T, int *counts,
                                   double *head, double *dt, double *acc, double *gyr, double *params, LfvioViAlignOut *out, double *x) {
  const WindowEstimator::LastViAlign &v = E(h)->last_vi_align;
  const int F = (int)v.stamps.size(), S = (int)v.dt.size();
  info[0] = F, info[1] = S, info[2] = v.called ? 1 : 0, info[3] = v.rc;
  const size_t f = (size_t)std::min(F, cap_frames), s = (size_t)std::min(S, cap_samples);
  if (stamps && f) std::memcpy(stamps, v.stamps.data(), f * 8);
  if (R && f) std::memcpy(R, v.R.data(), f * 72);
  if (T && f) std::memcpy(T, v.T.data(), f * 24);
  if (counts && f) std::memcpy(counts, v.counts.data(), f * 4);
  if (head && f) std::memcpy(head, v.head.data(), f * 96);
  if (dt && s) std::memcpy(dt, v.dt.data(), s * 8);
  if (acc && s) std::memcpy(acc, v.acc.data(), s * 24);
  if (gyr && s) std::memcpy(gyr, v.gyr.data(), s * 24);
  if (params) std::memcpy(params, v.noise, 32), std::memcpy(params + 4, v.tic, 24), params[7] = v.g_norm;
  if (out) *out = v.out;
  if (x && f && v.x.size() >= 3 * f) std::memcpy(x, v.x.data(), f * 24);
  return E(h)->vi_align_calls;
}
// tests: processImage() returns right behind a successful visualInitialAlign(), the window as the alignment left it (still
// initializing: no optimization(), no slide); gravity as aligned: lfvio_host_get_gravity
void lfvio_host_set_stop_after_align(void *h, int on) { E(h)->stop_after_align = on != 0; }
void lfvio_host_get_gravity(void *h, double *g) {
  for (int k = 0; k < 3; k++) g[k] = E(h)->g(k);
}
// out[2] = {attempts that reached the device, attempts that aligned}
void lfvio_host_vi_align_counts(void *h, long long *out) { out[0] = E(h)->vi_align_calls, out[1] = E(h)->vi_align_ok; }
// the SfM records of a trace file: stamps[cap] of the records, frames[cap] in each; returns their number, -1: unreadable
int lfvio_host_trace_sfms(const char *trace_path, int cap, double *stamps, int *frames, double *first_R, double *first_T, int cap_first) {
  Trace trace;
  if (!trace.load(trace_path)) return -1;
  for (int k = 0; k < (int)trace.sfms.size() && k < cap; k++) stamps[k] = trace.sfms[k].stamp, frames[k] = (int)trace.sfms[k].sfm.stamps.size();
  if (!trace.sfms.empty() && first_R && first_T) {
    const size_t n = std::min(trace.sfms[0].sfm.stamps.size(), (size_t)cap_first);
    std::memcpy(first_R, trace.sfms[0].sfm.R.data(), n * 72), std::memcpy(first_T, trace.sfms[0].sfm.T.data(), n * 24);
  }
  return (int)trace.sfms.size();
}

// the SfM structure records of a trace file: stamps[cap] of the records, counts[cap][2] = {keyframes, points} in each; of the
// first record (any may be null) kf[cap_kf][8] = {stamp, q w x y z, T} and pts[cap_pts][4] = {id, xyz}; returns their number, -1: unreadable
int lfvio_host_trace_structures(const char *trace_path, int cap, double *stamps, int *counts, double *kf, int cap_kf, double *pts, int cap_pts) {
  Trace trace;
  if (!trace.load(trace_path)) return -1;
  const std::vector<TraceStructure> &v = trace.structures;
  for (int k = 0; k < (int)v.size() && k < cap; k++) stamps[k] = v[k].stamp, counts[2 * k] = (int)v[k].st.stamps.size(), counts[2 * k + 1] = (int)v[k].st.ids.size();
  if (!v.empty()) {
    const WindowEstimator::SfmStructure &s = v[0].st;
    for (size_t k = 0; kf && k < s.stamps.size() && k < (size_t)cap_kf; k++) {
      kf[8 * k] = s.stamps[k];
      std::memcpy(kf + 8 * k + 1, &s.Q[4 * k], 32), std::memcpy(kf + 8 * k + 5, &s.T[3 * k], 24);
    }
    for (size_t k = 0; pts && k < s.ids.size() && k < (size_t)cap_pts; k++) {
      pts[4 * k] = s.ids[k];
      std::memcpy(pts + 4 * k + 1, &s.xyz[3 * k], 24);
    }
  }
  return (int)v.size();
}

int lfvio_host_optimization(void *h) {
  WindowEstimator *e = E(h);
  e->optimization();
  return e->status;
}
int lfvio_host_last_iterations(void *h) { return E(h)->summary.num_iterations; }
double lfvio_host_last_cost(void *h) { return E(h)->summary.final_cost; }

}  // extern "C"
