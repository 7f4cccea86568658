// window_estimator.cpp — see window_estimator.h.  Reference lines are relative to /root/reference/vins_estimator/src.
#include "window_estimator.h"
// A weak reference: the host sources are also linked against a C-ABI that has no relocalization entry point (the CPU oracle of
// the tests, oracle/abi_shim.cpp); there optimization() with a relocalization message reports LFVIO_ERR_DEVICE instead of loading
// with an unresolved symbol.
#pragma weak lfvio_solve_relo
// ... nor a two-view entry point: there ESTIMATE_EXTRINSIC == 2 reports LFVIO_ERR_DEVICE on the first image that needs it.
#pragma weak lfvio_two_view
#pragma weak lfvio_vi_align
#pragma weak lfvio_pnp
#pragma weak lfvio_sfm_construct
#pragma weak lfvio_sfm_ba
#pragma weak lfvio_relative_pose

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <numeric>

namespace lfvio {

Config &config() {
  static Config c;
  return c;
}

Vector3d yawPitchRollDeg(const Matrix3d &R) {  // utility.h:66-83
  const Vector3d n = R.col(0), o = R.col(1), a = R.col(2);
  const double y = atan2(n(1), n(0));
  const double p = atan2(-n(2), n(0) * cos(y) + n(1) * sin(y));
  const double r = atan2(a(0) * sin(y) - a(1) * cos(y), -o(0) * sin(y) + o(1) * cos(y));
  return Vector3d(y / M_PI * 180.0, p / M_PI * 180.0, r / M_PI * 180.0);
}

Matrix3d fromYawPitchRollDeg(const Vector3d &ypr) {  // utility.h:85-113
  const double y = ypr(0) / 180.0 * M_PI, p = ypr(1) / 180.0 * M_PI, r = ypr(2) / 180.0 * M_PI;
  Matrix3d Rz, Ry, Rx;
  Rz(0, 0) = cos(y), Rz(0, 1) = -sin(y), Rz(1, 0) = sin(y), Rz(1, 1) = cos(y), Rz(2, 2) = 1;
  Ry(0, 0) = cos(p), Ry(0, 2) = sin(p), Ry(1, 1) = 1, Ry(2, 0) = -sin(p), Ry(2, 2) = cos(p);
  Rx(0, 0) = 1, Rx(1, 1) = cos(r), Rx(1, 2) = -sin(r), Rx(2, 1) = sin(r), Rx(2, 2) = cos(r);
  return Rz * Ry * Rx;
}

// ---------------------------------------------------------------------------------------------------- ImuSpan
void ImuSpan::open(const Vector3d &a0, const Vector3d &g0, const Vector3d &ba, const Vector3d &bg) {
  close();
  present = true;
  for (int k = 0; k < 3; k++) acc0[k] = a0(k), gyr0[k] = g0(k), lin_ba[k] = ba(k), lin_bg[k] = bg(k);
  // an IntegrationBase without samples: identity Jacobian, zero covariance (integration_base.h:13-28)
  std::memset(&pre, 0, sizeof pre);
  pre.delta_q[3] = 1.0;
  for (int k = 0; k < 15; k++) pre.jacobian[16 * k] = 1.0;
  for (int k = 0; k < 3; k++) pre.linearized_ba[k] = lin_ba[k], pre.linearized_bg[k] = lin_bg[k];
}

void ImuSpan::push(double d, const double *a, const double *g) {
  dt.push_back(d);
  acc.insert(acc.end(), a, a + 3);
  gyr.insert(gyr.end(), g, g + 3);
  sum_dt += d;
  dirty = true;
}

// ---------------------------------------------------------------------------------------------------- TrackTable
void TrackTable::clear() {
  id_.clear(), start_.clear(), count_.clear(), first_.clear(), flag_.clear(), dead_.clear();
  depth_.clear(), rows_.clear(), order_.clear(), free_.clear(), slot_of_.clear();
  holes_ = false;
}

int TrackTable::solvableCount() const {
  int n = 0;
  for (int s : order_) n += solvable(s);
  return n;
}

int TrackTable::find(int feature_id) const {
  auto it = slot_of_.find(feature_id);
  return it == slot_of_.end() ? -1 : it->second;
}

int TrackTable::create(int feature_id, int start_frame) {
  int s;
  if (!free_.empty()) {
    s = free_.back();
    free_.pop_back();
  } else {
    s = (int)id_.size();
    id_.push_back(0), start_.push_back(0), count_.push_back(0), first_.push_back(0), flag_.push_back(0), dead_.push_back(0);
    depth_.push_back(0.0);
    rows_.resize(rows_.size() + (size_t)FRAMES * OBS_W);
  }
  id_[s] = feature_id, start_[s] = start_frame, count_[s] = 0, first_[s] = 0, flag_[s] = 0, dead_[s] = 0;
  depth_[s] = -1.0;  // FeaturePerId: estimated_depth(-1.0), solve_flag(0) (feature_manager.h:60-63)
  slot_of_[feature_id] = s;
  order_.push_back(s);
  return s;
}

void TrackTable::append(int s, const double *pt8, double cur_td) {
  if (count_[s] >= FRAMES) return;  // a track cannot be longer than the window
  double *r = &rows_[((size_t)s * FRAMES + (first_[s] + count_[s]) % FRAMES) * OBS_W];
  std::memcpy(r, pt8, 8 * sizeof(double));
  r[8] = cur_td;
  count_[s]++;
}

int TrackTable::corresponding(int l, int r, std::vector<double> *bl, std::vector<double> *br) const {  // feature_manager.cpp:118-137
  bl->clear(), br->clear();
  for (int s : order_) {
    if (!(start_[s] <= l && start_[s] + count_[s] - 1 >= r)) continue;
    const double *a = obs(s, l - start_[s]), *b = obs(s, r - start_[s]);
    bl->insert(bl->end(), a, a + 3), br->insert(br->end(), b, b + 3);
  }
  return (int)bl->size() / 3;
}

int TrackTable::appendFrame(int frame_count, int n, const int *ids, const double *pts8, double td) {
  // the reference walks a std::map keyed by feature id (estimator_node.cpp:292-312): ascending ids, and of several
  // entries with one id only the first is used (id_pts.second[0])
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return ids[a] < ids[b]; });
  int continued = 0;
  for (int k = 0; k < n; k++) {
    const int i = idx[k];
    if (k > 0 && ids[idx[k - 1]] == ids[i]) continue;
    int s = find(ids[i]);
    if (s < 0) {
      s = create(ids[i], frame_count);
    } else {
      continued++;
    }
    append(s, pts8 + 8 * (size_t)i, td);
  }
  return continued;
}

void TrackTable::parallax(int frame_count, double *sum, int *num) const {
  double acc = 0;
  int cnt = 0;
  for (int s : order_) {
    if (!(start_[s] <= frame_count - 2 && start_[s] + count_[s] - 1 >= frame_count - 1)) continue;
    const double *pi = obs(s, frame_count - 2 - start_[s]), *pj = obs(s, frame_count - 1 - start_[s]);
    acc += acos(pi[0] * pj[0] + pi[1] * pj[1] + pi[2] * pj[2]) * 10;  // the angle between the two bearings, uncompensated
    cnt++;
  }
  *sum = acc, *num = cnt;
}

void TrackTable::erase(int s) {
  dead_[s] = 1;
  slot_of_.erase(id_[s]);
  free_.push_back(s);
  holes_ = true;
}

void TrackTable::compact() {
  if (!holes_) return;
  order_.erase(std::remove_if(order_.begin(), order_.end(), [&](int s) { return dead_[s] != 0; }), order_.end());
  holes_ = false;
}

void TrackTable::dropOldestFrame(std::vector<Shifted> *survivors) {
  for (int s : order_) {
    if (start_[s] != 0) {
      start_[s]--;
      continue;
    }
    const double *b = obs(s, 0);
    Shifted sh{s, {b[0], b[1], b[2]}};
    first_[s] = (first_[s] + 1) % FRAMES;  // the row stays where it is; the track just starts one row later
    count_[s]--;
    if (survivors) {
      if (count_[s] < 2) erase(s);
      else survivors->push_back(sh);
    } else if (count_[s] == 0) {
      erase(s);
    }
  }
  compact();
}

void TrackTable::dropSecondNewestFrame(int frame_count) {
  for (int s : order_) {
    if (start_[s] == frame_count) {
      start_[s]--;
      continue;
    }
    if (start_[s] + count_[s] - 1 < frame_count - 1) continue;
    const int j = WINDOW_SIZE - 1 - start_[s];
    // at most the newest frame's observation sits behind row j
    for (int k = j; k + 1 < count_[s]; k++)
      std::memcpy(const_cast<double *>(obs(s, k)), obs(s, k + 1), OBS_W * sizeof(double));
    if (--count_[s] == 0) erase(s);
  }
  compact();
}

void TrackTable::dropFailed() {
  for (int s : order_)
    if (flag_[s] == 2) erase(s);
  compact();
}

// ---------------------------------------------------------------------------------------------------- WindowEstimator
WindowEstimator::WindowEstimator() {
  std::memset(&summary, 0, sizeof summary);
  std::memset(&prior, 0, sizeof prior);
  std::memset(&next_, 0, sizeof next_);
  reset();
}

WindowEstimator::~WindowEstimator() {
  if (group) lfvio_group_destroy(group);  // owns its contexts, `gpu` among them
  else if (gpu) lfvio_destroy(gpu);
}

namespace {
// what is there of a prior: header, n x n of the Jacobian slots, n residuals (46 KB instead of 240 KB for n = 76)
void assign_prior(LfvioPrior *dst, const LfvioPrior *src) {
  std::memcpy(dst, src, offsetof(LfvioPrior, linearized_jacobians));
  if (src->valid && src->n > 0 && src->n <= LFVIO_MAX_PRIOR_DIM) {
    std::memcpy(dst->linearized_jacobians, src->linearized_jacobians, sizeof(double) * src->n * src->n);
    std::memcpy(dst->linearized_residuals, src->linearized_residuals, sizeof(double) * src->n);
  }
}
}  // namespace

// The marginalization of the last optimization() may still be running on the device (Config::split_call): wait for it and
// adopt its prior.  Everything that reads `prior` starts here.
namespace {
struct Stopwatch {  // adds its lifetime to *acc
  double *acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit Stopwatch(double *a) : acc(a) {}
  ~Stopwatch() { *acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

bool WindowEstimator::collectPrior() {
  if (!prior_pending_) return true;
  Stopwatch sw(&timers[1]);
  prior_pending_ = false;
  const int rc = lfvio_batch_optimize_finish(gpu, &next_);
  if (rc != LFVIO_OK) {
    status = rc;
    return false;
  }
  assign_prior(&prior, &next_), has_prior = next_.valid != 0;
  return true;
}

bool WindowEstimator::device() {
  if (!gpu) {
    const unsigned mask = config().device_mask ? config().device_mask : 1u;
    if (config().local_shards > 1) {
      int d = 0;
      while (!(mask & (1u << d))) d++;
      group = lfvio_group_create_local(d, config().local_shards);
      gpu = group ? lfvio_group_ctx(group, 0) : nullptr;
    } else if (mask & (mask - 1)) {  // several devices: one group, whose first context also serves the single-device calls
      group = lfvio_group_create(mask);
      gpu = group ? lfvio_group_ctx(group, 0) : nullptr;
    } else {
      int d = 0;
      while (!(mask & (1u << d))) d++;
      gpu = lfvio_create(d);
    }
  }
  if (!gpu) status = LFVIO_ERR_DEVICE;  // there is no host fallback: the caller sees the failure
  return gpu != nullptr;
}

void WindowEstimator::reset() {
  // clearState() (estimator.cpp:23-84) followed by setParameter() (:10-21): the CONFIGURED extrinsic and td come back,
  // and a bootstrap record that described the old window is not reused
  const Config &c = config();
  if (prior_pending_) {  // the prior of a window that is being dropped: wait for the device, keep nothing
    prior_pending_ = false;
    (void)lfvio_batch_optimize_finish(gpu, nullptr);
  }
  ring_.head = 0;
  for (int i = 0; i < FRAMES; i++) {
    frames_[i] = Keyframe();
    frames_[i].R.setIdentity();
    spans_[i].close();
  }
  for (int k = 0; k < 3; k++) tic(k) = c.tic[k];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) ric(i, j) = c.ric[3 * i + j];
  td = c.td;
  phase = INITIAL;
  first_imu = false;
  relocalization_info = 0;
  slides_old = slides_new = 0;
  frame_count = 0;
  initial_timestamp = 0;
  has_prior = false;
  tracks.clear();
  failure_occur = false;
  bootstrap.valid = false;
  bootstrap.depth_ids.clear(), bootstrap.depths.clear();
  sfm.valid = false;
  structure.valid = false;
  relative.valid = false;
  image_frames.clear();  // clearState(): all_image_frame.clear(), tmp_pre_integration = nullptr (estimator.cpp:60-66)
  pending_ = ImageFrame();
}

void WindowEstimator::pushImu(double dt, const double acc[3], const double gyr[3]) {  // estimator.cpp:86-120
  const Vector3d a(acc[0], acc[1], acc[2]), w(gyr[0], gyr[1], gyr[2]);
  if (!first_imu) {
    first_imu = true;
    acc_prev = a, gyr_prev = w;
  }
  Keyframe &f = kf(frame_count);
  ImuSpan &sp = span(frame_count);
  if (!sp.present) sp.open(acc_prev, gyr_prev, f.Ba, f.Bg);
  if (frame_count != 0) {
    sp.push(dt, acc, gyr);
    pending_.dt.push_back(dt), pending_.acc.insert(pending_.acc.end(), acc, acc + 3), pending_.gyr.insert(pending_.gyr.end(), gyr, gyr + 3);  // :103
    // mid-point dead reckoning of the newest keyframe
    const Vector3d a0 = f.R * (acc_prev - f.Ba) - g;
    const Vector3d wm = 0.5 * (gyr_prev + w) - f.Bg;
    f.R = f.R * Quaterniond(1.0, wm(0) * dt / 2.0, wm(1) * dt / 2.0, wm(2) * dt / 2.0).toRotationMatrix();  // Utility::deltaQ, unnormalised
    const Vector3d a1 = f.R * (a - f.Ba) - g;
    const Vector3d am = 0.5 * (a0 + a1);
    f.P += dt * f.V + 0.5 * dt * dt * am;
    f.V += dt * am;
  }
  acc_prev = a, gyr_prev = w;
}

bool WindowEstimator::keyframeTest(int fc, int n, const int *ids, const double *pts8, double cur_td) {  // feature_manager.cpp:45-95
  tracked_last = tracks.appendFrame(fc, n, ids, pts8, cur_td);
  if (fc < 2 || tracked_last < 20) return true;
  double sum;
  int num;
  tracks.parallax(fc, &sum, &num);
  if (num == 0) return true;
  return sum / num >= config().min_parallax;
}

bool WindowEstimator::applyBootstrap() {
  // stand-in for initialStructure() + visualInitialAlign() (estimator.cpp:222-473): the aligned window state comes from the
  // record; what the reference does with it afterwards is kept: every span is integrated again with its new gyroscope bias
  // and a zero accelerometer bias (:403-406), gravity is taken over (:445), every depth is marked unknown (:386-390)
  if (!bootstrap.valid) return false;
  for (int i = 0; i < FRAMES; i++) {
    const double stamp = kf(i).stamp;
    kf(i) = bootstrap.kf[i];
    kf(i).stamp = stamp;
  }
  g = bootstrap.g;
  Vector3d zero[FRAMES], bg[FRAMES];
  for (int i = 0; i < FRAMES; i++) bg[i] = kf(i).Bg;
  if (!refreshSpans(true, zero, bg)) return false;
  for (int s : tracks.order()) tracks.setDepth(s, -1.0);
  for (size_t k = 0; k < bootstrap.depth_ids.size() && k < bootstrap.depths.size(); k++) {
    const int s = tracks.find(bootstrap.depth_ids[k]);
    if (s >= 0) tracks.setDepth(s, bootstrap.depths[k]);
  }
  return true;
}

namespace {
Matrix3d g2R(const Vector3d &g) {  // Utility::g2R (utility.cpp:3-13): FromTwoVectors(g / |g|, z), its yaw taken out
  const Vector3d v0 = g / g.norm(), v1(0, 0, 1);
  const double c = v1.dot(v0);
  Quaterniond q;
  if (c < -1.0 + 1e-12) {  // antiparallel (Eigen takes the axis from an SVD there): half a turn about x
    q = Quaterniond(0, 1, 0, 0);
  } else {
    const Vector3d axis(v0.y() * v1.z() - v0.z() * v1.y(), v0.z() * v1.x() - v0.x() * v1.z(), v0.x() * v1.y() - v0.y() * v1.x());
    const double s = std::sqrt((1.0 + c) * 2.0), invs = 1.0 / s;
    q = Quaterniond(s * 0.5, axis.x() * invs, axis.y() * invs, axis.z() * invs);
  }
  const Matrix3d R0 = q.toRotationMatrix();
  const double yaw = yawPitchRollDeg(R0).x();
  return fromYawPitchRollDeg(Vector3d(-yaw, 0, 0)) * R0;
}
}  // namespace

bool WindowEstimator::relativePose() {  // estimator.cpp:445-473
  LastRelative &lr = last_relative;
  lr.called = false, lr.rc = LFVIO_OK;
  lr.offset.assign(1, 0), lr.bl.clear(), lr.br.clear();
  std::memset(&lr.out, 0, sizeof lr.out);
  lr.out.l = -1;
  relative.valid = false;
  const int S = std::max(1, config().ransac_iterations);
  lr.num_samples = S;
  lr.samples.assign((size_t)WINDOW_SIZE * S * 8, 0);
  std::vector<double> bl, br;
  bool fits = true;
  for (int i = 0; i < WINDOW_SIZE; i++) {  // :448-451
    const int N = tracks.corresponding(i, WINDOW_SIZE, &bl, &br);
    lr.bl.insert(lr.bl.end(), bl.begin(), bl.end()), lr.br.insert(lr.br.end(), br.begin(), br.end());
    lr.offset.push_back(lr.offset.back() + N);
    fits = fits && N <= 4096;  // (the device entry's limit)
  }
  if (!fits || lr.offset.back() == 0) return false;  // (no match at all: every pair is skipped, :452)
  if (!lfvio_relative_pose || !device()) {  // no fallback: over an ABI without the entry the attempt fails
    status = LFVIO_ERR_DEVICE;
    lr.rc = LFVIO_ERR_DEVICE;
    return false;
  }
  seedRansac();
  for (int i = 0; i < WINDOW_SIZE; i++) {  // util::create_random_array per iteration of myfindFundamentalMat (solve_5pts.cpp:300)
    const int N = lr.offset[i + 1] - lr.offset[i];
    if (N <= 20) continue;  // :452
    for (int k = 0; k < S; k++) drawSampleSet(ransac_rng_, N, &lr.samples[((size_t)i * S + k) * 8]);
  }
  LfvioRelativePoseIn in;
  in.num_pairs = WINDOW_SIZE, in.match_offset = lr.offset.data(), in.bearing_l = lr.bl.data(), in.bearing_r = lr.br.data();
  in.num_samples = S, in.samples = lr.samples.data();
  lr.rc = lfvio_relative_pose(gpu, &in, nullptr, &lr.out);
  lr.called = true;
  relative_calls++;
  if (lr.rc != LFVIO_OK) {
    status = lr.rc;
    return false;
  }
  if (lr.out.l < 0) return false;  // :472
  relative.l = lr.out.l;
  std::memcpy(relative.R, lr.out.relative_R, sizeof relative.R), std::memcpy(relative.T, lr.out.relative_T, sizeof relative.T);
  relative.valid = true;
  relative_ok++;
  return true;
}

bool WindowEstimator::constructSfm() {  // estimator.cpp:250-286
  LastConstruct &lc = last_construct;
  lc.called = lc.ba_called = false, lc.rc = lc.ba_rc = LFVIO_OK;
  lc.ids.clear(), lc.offset.assign(1, 0), lc.frame.clear(), lc.bearing.clear();
  lc.c_rotation.clear(), lc.c_translation.clear(), lc.position.clear(), lc.tri_op.clear();
  std::memset(&lc.out, 0, sizeof lc.out), std::memset(&lc.ba, 0, sizeof lc.ba);
  structure.valid = false;
  const int F = frame_count + 1, l = relative.l;
  lc.F = F, lc.l = l;
  std::memcpy(lc.R, relative.R, sizeof lc.R), std::memcpy(lc.T, relative.T, sizeof lc.T);
  if (F < 2 || F > LFVIO_NUM_FRAMES || l < 0 || l > F - 2) return false;
  for (int s : tracks.order()) {  // :255-269
    const int start = tracks.start(s), n = tracks.count(s);
    if (n < 1 || start < 0 || start + n > F) return false;
    lc.ids.push_back(tracks.id(s));
    for (int k = 0; k < n; k++) {
      lc.frame.push_back(start + k);
      const double *o = tracks.obs(s, k);
      lc.bearing.insert(lc.bearing.end(), o, o + 3);
    }
    lc.offset.push_back((int)lc.frame.size());
  }
  const int P = (int)lc.ids.size();
  if (P < 1 || P > 4096) return false;  // (4096: the device entries' limit)
  if (!lfvio_sfm_construct || !lfvio_sfm_ba || !device()) {  // no fallback: over an ABI without the entries the attempt fails
    status = LFVIO_ERR_DEVICE;
    lc.rc = LFVIO_ERR_DEVICE;
    return false;
  }
  lc.c_rotation.assign(4 * (size_t)F, 0.0), lc.c_translation.assign(3 * (size_t)F, 0.0), lc.position.assign(3 * (size_t)P, 0.0), lc.tri_op.assign(P, -1);
  LfvioSfmConstructIn in;
  in.num_frames = F, in.ref_frame = l, in.num_points = P;
  in.obs_offset = lc.offset.data(), in.obs_frame = lc.frame.data(), in.obs_bearing = lc.bearing.data();
  std::memcpy(in.relative_R, relative.R, sizeof in.relative_R), std::memcpy(in.relative_T, relative.T, sizeof in.relative_T);
  lc.rc = lfvio_sfm_construct(gpu, &in, lc.c_rotation.data(), lc.c_translation.data(), lc.position.data(), lc.tri_op.data(), &lc.out);
  lc.called = true;
  construct_calls++;
  if (lc.rc != LFVIO_OK) {
    status = lc.rc;
    return false;
  }
  if (lc.out.status != 0 || lc.out.num_triangulated < 1) return false;
  // :259-275: the entries with state == true, in sfm_f order
  std::vector<int> keep, off(1, 0), frm;
  std::vector<double> us, X, q = lc.c_rotation, t = lc.c_translation;
  for (int j = 0; j < P; j++) {
    if (lc.tri_op[j] < 0) continue;
    keep.push_back(j);
    frm.insert(frm.end(), lc.frame.begin() + lc.offset[j], lc.frame.begin() + lc.offset[j + 1]);
    us.insert(us.end(), lc.bearing.begin() + 3 * (size_t)lc.offset[j], lc.bearing.begin() + 3 * (size_t)lc.offset[j + 1]);
    X.insert(X.end(), &lc.position[3 * (size_t)j], &lc.position[3 * (size_t)j] + 3);
    off.push_back((int)frm.size());
  }
  LfvioSfmBaIn bin;
  bin.num_frames = F, bin.ref_frame = l, bin.num_points = (int)keep.size();
  bin.obs_offset = off.data(), bin.obs_frame = frm.data(), bin.obs_bearing = us.data();
  bin.max_num_iterations = -1, bin.function_tolerance = bin.gradient_tolerance = bin.parameter_tolerance = 0.0;  // Ceres' defaults (:276-281)
  lc.ba_rc = lfvio_sfm_ba(gpu, &bin, q.data(), t.data(), X.data(), &lc.ba);
  lc.ba_called = true;
  if (lc.ba_rc != LFVIO_OK) {
    status = lc.ba_rc;
    return false;
  }
  if (!lc.ba.accepted) return false;  // :283-294
  SfmStructure &st = structure;  // :295-314
  st.stamps.resize(F), st.Q.resize(4 * (size_t)F), st.T.resize(3 * (size_t)F);
  for (int i = 0; i < F; i++) {
    st.stamps[i] = kf(i).stamp;
    std::memcpy(&st.Q[4 * (size_t)i], lc.ba.Q[i], 32), std::memcpy(&st.T[3 * (size_t)i], lc.ba.T[i], 24);
  }
  st.ids.resize(keep.size());
  for (size_t k = 0; k < keep.size(); k++) st.ids[k] = lc.ids[keep[k]];
  st.xyz = X;
  st.valid = true;
  construct_ok++;
  return true;
}

bool WindowEstimator::solvePnpFrames() {  // estimator.cpp:288-357
  const Config &c = config();
  LastPnp &lp = last_pnp;
  lp.called = false, lp.rc = LFVIO_OK;
  lp.stamps.clear(), lp.offset.assign(1, 0), lp.pw.clear(), lp.us.clear(), lp.out.clear();
  sfm.valid = false;
  const SfmStructure &st = structure;
  const int F = (int)image_frames.size(), K = (int)st.stamps.size();
  if (F < 1 || F > LFVIO_MAX_IMAGE_FRAMES || st.Q.size() < 4 * (size_t)K || st.T.size() < 3 * (size_t)K || st.xyz.size() < 3 * st.ids.size()) return false;
  Matrix3d RIC;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) RIC(i, j) = c.ric[3 * i + j];
  // every keyframe of the window must be in the structure
  for (int i = 0; i <= frame_count; i++)
    if (std::find(st.stamps.begin(), st.stamps.end(), kf(i).stamp) == st.stamps.end()) return false;
  std::vector<int> by_id(st.ids.size());  // sfm_tracked_points.find()
  std::iota(by_id.begin(), by_id.end(), 0);
  std::sort(by_id.begin(), by_id.end(), [&](int a, int b) { return st.ids[a] < st.ids[b]; });
  auto findPoint = [&](int id) {
    auto it = std::lower_bound(by_id.begin(), by_id.end(), id, [&](int a, int v) { return st.ids[a] < v; });
    return it != by_id.end() && st.ids[*it] == id ? *it : -1;
  };
  sfm.stamps.assign(F, 0.0), sfm.R.assign(9 * (size_t)F, 0.0), sfm.T.assign(3 * (size_t)F, 0.0);
  std::vector<int> frame_of;  // list index of each non-keyframe
  for (int k = 0; k < F; k++) {
    const ImageFrame &f = image_frames[k];
    sfm.stamps[k] = f.stamp;
    bool key = false;
    for (int i = 0; i <= frame_count; i++) key = key || kf(i).stamp == f.stamp;
    if (key) {  // :296-303
      const int j = (int)(std::find(st.stamps.begin(), st.stamps.end(), f.stamp) - st.stamps.begin());
      const Matrix3d R = Quaterniond(st.Q[4 * j], st.Q[4 * j + 1], st.Q[4 * j + 2], st.Q[4 * j + 3]).toRotationMatrix() * RIC.transpose();
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) sfm.R[9 * (size_t)k + 3 * a + b] = R(a, b);
      std::memcpy(&sfm.T[3 * (size_t)k], &st.T[3 * (size_t)j], 24);
      continue;
    }
    for (size_t m = 0; m < f.ids.size(); m++) {  // :318-333
      const int p = findPoint(f.ids[m]);
      if (p < 0) continue;
      lp.us.insert(lp.us.end(), &f.pts[3 * m], &f.pts[3 * m] + 3);
      lp.pw.insert(lp.pw.end(), &st.xyz[3 * (size_t)p], &st.xyz[3 * (size_t)p] + 3);
    }
    const int n = (int)(lp.us.size() / 3) - lp.offset.back();
    lp.stamps.push_back(f.stamp), lp.offset.push_back(lp.offset.back() + n), frame_of.push_back(k);
    if (n < 6 || n > 4096) return false;  // :335-340 "Not enough points for solve pnp !" (4096: the device entry's limit)
  }
  const int NF = (int)frame_of.size();
  if (NF > 0) {
    if (!lfvio_pnp || !device()) {  // no fallback: over an ABI without the entry the attempt fails and the window slides
      status = LFVIO_ERR_DEVICE;
      lp.rc = LFVIO_ERR_DEVICE;
      return false;
    }
    lp.out.resize(NF);
    std::memset(lp.out.data(), 0, sizeof(LfvioPnpOut) * (size_t)NF);
    LfvioPnpIn in;
    in.num_frames = NF, in.offset = lp.offset.data(), in.point_w = lp.pw.data(), in.bearing = lp.us.data();
    lp.rc = lfvio_pnp(gpu, &in, lp.out.data());
    lp.called = true;
    pnp_calls++;
    if (lp.rc != LFVIO_OK) {
      status = lp.rc;
      return false;
    }
    for (int q = 0; q < NF; q++) {
      const LfvioPnpOut &o = lp.out[q];
      if (o.status != 0) return false;
      Matrix3d tmp;
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) tmp(a, b) = o.R[3 * a + b];
      const Matrix3d R_pnp = tmp.transpose();                             // :353
      const Vector3d T_pnp = R_pnp * (-Vector3d(o.T[0], o.T[1], o.T[2]));  // :354
      const Matrix3d R = R_pnp * RIC.transpose();                         // :355
      const int k = frame_of[q];
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) sfm.R[9 * (size_t)k + 3 * a + b] = R(a, b);
      for (int a = 0; a < 3; a++) sfm.T[3 * (size_t)k + a] = T_pnp(a);
    }
  }
  sfm.valid = true;
  return true;
}

bool WindowEstimator::visualInitialAlign() {  // estimator.cpp:367-443 on the SfM poses of `sfm`; VisualIMUAlignment on the device
  const Config &c = config();
  LastViAlign &lv = last_vi_align;
  lv.called = false;
  const int F = (int)image_frames.size();
  if (F < 1 || F > LFVIO_MAX_IMAGE_FRAMES) return false;
  // ImageFrame::R, T of every frame of the list, by stamp; a frame the result does not cover: no attempt
  lv.stamps.assign(F, 0.0), lv.R.assign(9 * (size_t)F, 0.0), lv.T.assign(3 * (size_t)F, 0.0);
  for (int k = 0; k < F; k++) {
    size_t j = 0;
    while (j < sfm.stamps.size() && sfm.stamps[j] != image_frames[k].stamp) j++;
    if (j == sfm.stamps.size() || sfm.R.size() < 9 * (j + 1) || sfm.T.size() < 3 * (j + 1)) return false;
    lv.stamps[k] = image_frames[k].stamp;
    std::memcpy(&lv.R[9 * (size_t)k], &sfm.R[9 * j], 72), std::memcpy(&lv.T[3 * (size_t)k], &sfm.T[3 * j], 24);
  }
  std::vector<LfvioImuInterval> spans(F);
  lv.counts.assign(F, 0), lv.head.assign(12 * (size_t)F, 0.0), lv.dt.clear(), lv.acc.clear(), lv.gyr.clear();
  for (int k = 0; k < F; k++) {
    const ImageFrame &f = image_frames[k];
    LfvioImuInterval &iv = spans[k];
    std::memset(&iv, 0, sizeof iv);
    if (k == 0) continue;  // span[0] is not read
    iv.num_samples = (int)f.dt.size(), iv.dt = f.dt.data(), iv.acc = f.acc.data(), iv.gyr = f.gyr.data();
    std::memcpy(iv.acc_0, f.acc0, 24), std::memcpy(iv.gyr_0, f.gyr0, 24), std::memcpy(iv.linearized_ba, f.lin_ba, 24), std::memcpy(iv.linearized_bg, f.lin_bg, 24);
    lv.counts[k] = iv.num_samples;
    std::memcpy(&lv.head[12 * (size_t)k], f.lin_ba, 24), std::memcpy(&lv.head[12 * (size_t)k + 3], f.lin_bg, 24);
    std::memcpy(&lv.head[12 * (size_t)k + 6], f.acc0, 24), std::memcpy(&lv.head[12 * (size_t)k + 9], f.gyr0, 24);
    lv.dt.insert(lv.dt.end(), f.dt.begin(), f.dt.end()), lv.acc.insert(lv.acc.end(), f.acc.begin(), f.acc.end()), lv.gyr.insert(lv.gyr.end(), f.gyr.begin(), f.gyr.end());
  }
  LfvioViAlignIn in;
  in.num_frames = F, in.R = lv.R.data(), in.T = lv.T.data(), in.span = spans.data();
  in.noise[0] = c.acc_n, in.noise[1] = c.gyr_n, in.noise[2] = c.acc_w, in.noise[3] = c.gyr_w;
  const Vector3d G(c.gravity[0], c.gravity[1], c.gravity[2]);
  for (int k = 0; k < 3; k++) in.tic[k] = c.tic[k];
  in.g_norm = G.norm();
  std::memcpy(lv.noise, in.noise, sizeof lv.noise), std::memcpy(lv.tic, in.tic, sizeof lv.tic), lv.g_norm = in.g_norm;
  std::memset(&lv.out, 0, sizeof lv.out);
  lv.x.assign(3 * (size_t)F, 0.0);
  if (!lfvio_vi_align || !device()) {  // no fallback: over an ABI without the entry the attempt fails and the window slides
    status = LFVIO_ERR_DEVICE;
    lv.rc = LFVIO_ERR_DEVICE;
    return false;
  }
  lv.rc = lfvio_vi_align(gpu, &in, &lv.out, lv.x.data(), nullptr);
  lv.called = true;
  vi_align_calls++;
  if (lv.rc != LFVIO_OK) {
    status = lv.rc;
    return false;
  }
  if (lv.out.status == 3) return false;  // (deviation of include/lfvio.h: nothing was computed)
  // solveGyroscopeBias has moved every Bgs and re-propagated every frame's integration before LinearAlignment can fail
  // (initial_aligment.cpp:28-35)
  const Vector3d dbg(lv.out.delta_bg[0], lv.out.delta_bg[1], lv.out.delta_bg[2]);
  for (int i = 0; i <= WINDOW_SIZE; i++) kf(i).Bg += dbg;
  for (int k = 1; k < F; k++)
    for (int d = 0; d < 3; d++) image_frames[k].lin_ba[d] = 0.0, image_frames[k].lin_bg[d] = kf(0).Bg(d);
  if (lv.out.status != 0) return false;
  auto frameOf = [&](double stamp) {
    int k = 0;
    while (k < F && image_frames[k].stamp != stamp) k++;
    return k;
  };
  for (int i = 0; i <= frame_count; i++) {  // :380-387
    const int k = frameOf(kf(i).stamp);
    if (k == F) return false;
    Keyframe &f = kf(i);
    f.P = Vector3d(lv.T[3 * k], lv.T[3 * k + 1], lv.T[3 * k + 2]);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) f.R(a, b) = lv.R[9 * (size_t)k + 3 * a + b];
  }
  for (int s : tracks.order())  // :389-392 (getDepthVector: the solvable tracks)
    if (tracks.solvable(s)) tracks.setDepth(s, -1.0);
  {  // :394-400: triangulate on camera poses, no tic, the configured ric
    const Vector3d tic_kept = tic;
    tic.setZero();
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) ric(i, j) = c.ric[3 * i + j];
    triangulate();
    tic = tic_kept;
    if (status != LFVIO_OK) return false;
  }
  const double s = lv.out.s;  // :402
  Vector3d zero[FRAMES], bg[FRAMES];
  for (int i = 0; i < FRAMES; i++) bg[i] = kf(i).Bg;
  if (!refreshSpans(true, zero, bg)) return false;  // :403-406
  const Vector3d TIC(c.tic[0], c.tic[1], c.tic[2]);
  for (int i = frame_count; i >= 0; i--) kf(i).P = s * kf(i).P - kf(i).R * TIC - (s * kf(0).P - kf(0).R * TIC);  // :407-408
  // :409-418, kept as written: kv counts KEYFRAMES but indexes x, which is laid out over ALL frames of the list — with a
  // non-keyframe in the list the later keyframes take the velocity solved for an earlier frame
  int kv = -1;
  for (int k = 0; k < F; k++) {
    bool key = false;
    for (int i = 0; i <= frame_count; i++) key = key || kf(i).stamp == image_frames[k].stamp;
    if (!key) continue;
    kv++;
    Matrix3d Rk;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) Rk(a, b) = lv.R[9 * (size_t)k + 3 * a + b];
    kf(kv).V = Rk * Vector3d(lv.x[3 * kv], lv.x[3 * kv + 1], lv.x[3 * kv + 2]);
  }
  for (int t : tracks.order())  // :419-425
    if (tracks.solvable(t)) tracks.setDepth(t, tracks.depth(t) * s);
  g = Vector3d(lv.out.g[0], lv.out.g[1], lv.out.g[2]);
  Matrix3d R0 = g2R(g);  // :427-438
  const double yaw = yawPitchRollDeg(R0 * kf(0).R).x();
  R0 = fromYawPitchRollDeg(Vector3d(-yaw, 0, 0)) * R0;
  g = R0 * g;
  for (int i = 0; i <= frame_count; i++) kf(i).P = R0 * kf(i).P, kf(i).R = R0 * kf(i).R, kf(i).V = R0 * kf(i).V;
  vi_align_ok++;
  return true;
}

// ---------------------------------------------------------------------------------------------------- ExRotationCalibrator
namespace {

Matrix3d inverse3(const Matrix3d &a) {  // by the adjugate
  Matrix3d r;
  r(0, 0) = a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), r(0, 1) = a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2), r(0, 2) = a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1);
  r(1, 0) = a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2), r(1, 1) = a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0), r(1, 2) = a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2);
  r(2, 0) = a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0), r(2, 1) = a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1), r(2, 2) = a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0);
  const double det = a(0, 0) * r(0, 0) + a(0, 1) * r(1, 0) + a(0, 2) * r(2, 0);
  return (1.0 / det) * r;
}

double angularDistance(const Quaterniond &a, const Quaterniond &b) {  // Eigen: 2 atan2(|vec|, |w|) of a * conj(b)
  const Quaterniond d = a * Quaterniond(b.w(), -b.x(), -b.y(), -b.z());
  return 2.0 * std::atan2(d.vec().norm(), std::abs(d.w()));
}

// singular values (falling) and right singular vectors of an m x 4 matrix (row-major, overwritten): one-sided Jacobi
void svd4(std::vector<double> &A, int m, double sv[4], double V[4][4]) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) V[i][j] = i == j;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < m; r++) {
          const double x = A[4 * r + p], y = A[4 * r + q];
          al += x * x, be += y * y, ga += x * y;
        }
        if (ga == 0.0 || std::abs(ga) <= 2.3e-16 * std::sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::abs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < m; r++) {
          const double x = A[4 * r + p], y = A[4 * r + q];
          A[4 * r + p] = c * x - s * y, A[4 * r + q] = s * x + c * y;
        }
        for (int r = 0; r < 4; r++) {
          const double x = V[r][p], y = V[r][q];
          V[r][p] = c * x - s * y, V[r][q] = s * x + c * y;
        }
      }
    if (!rotated) break;
  }
  double n[4];
  int order[4] = {0, 1, 2, 3};
  for (int c = 0; c < 4; c++) {
    double s = 0;
    for (int r = 0; r < m; r++) s += A[4 * r + c] * A[4 * r + c];
    n[c] = std::sqrt(s);
  }
  std::stable_sort(order, order + 4, [&](int a, int b) { return n[a] > n[b]; });
  double Vs[4][4];
  for (int c = 0; c < 4; c++) {
    sv[c] = n[order[c]];
    for (int r = 0; r < 4; r++) Vs[r][c] = V[r][order[c]];
  }
  std::memcpy(V, Vs, sizeof Vs);
}

}  // namespace

void ExRotationCalibrator::clear() {  // initial_ex_rotation.cpp:4-11
  frame_count = 0;
  Rc.assign(1, Matrix3d::Identity()), Rimu.assign(1, Matrix3d::Identity()), Rc_g.assign(1, Matrix3d::Identity());
  ric.setIdentity();
  sv[0] = sv[1] = sv[2] = sv[3] = 0;
}

bool ExRotationCalibrator::push(const Matrix3d &Rc_new, const Quaterniond &delta_q, Matrix3d *calib_ric) {  // :13-67
  frame_count++;
  Rc.push_back(Rc_new);
  Rimu.push_back(delta_q.toRotationMatrix());
  Rc_g.push_back(inverse3(ric) * delta_q.toRotationMatrix() * ric);
  std::vector<double> A((size_t)frame_count * 16, 0.0);
  for (int i = 1; i <= frame_count; i++) {
    const Quaterniond r1(Rc[i]), r2(Rc_g[i]);
    const double angular_distance = 180.0 / M_PI * angularDistance(r1, r2);
    const double huber = angular_distance > 5.0 ? 5.0 / angular_distance : 1.0;
    double L[4][4], R[4][4];
    auto fill = [](double M[4][4], double w, const Vector3d &q, double sgn) {  // w I +- [q]x | q ; -q^T | w
      const double sk[3][3] = {{0, -q.z(), q.y()}, {q.z(), 0, -q.x()}, {-q.y(), q.x(), 0}};
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) M[a][b] = (a == b ? w : 0.0) + sgn * sk[a][b];
        M[a][3] = q(a), M[3][a] = -q(a);
      }
      M[3][3] = w;
    };
    fill(L, r1.w(), r1.vec(), 1.0);
    const Quaterniond R_ij(Rimu[i]);
    fill(R, R_ij.w(), R_ij.vec(), -1.0);
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++) A[(size_t)(i - 1) * 16 + 4 * a + b] = huber * (L[a][b] - R[a][b]);
  }
  double V[4][4];
  svd4(A, 4 * frame_count, sv, V);
  const Quaterniond estimated_R(V[3][3], V[0][3], V[1][3], V[2][3]);  // x = V.col(3) holds (x, y, z, w)
  ric = inverse3(estimated_R.toRotationMatrix());
  if (frame_count >= WINDOW_SIZE && sv[2] > 0.25) {
    *calib_ric = ric;
    return true;
  }
  return false;
}

void drawSampleSet(std::mt19937 &rng, int n, int out[8]) {
  std::uniform_int_distribution<int> dist(0, n - 1);
  const size_t size = 8, make_size = 9;  // static_cast<size_t>(8 * 1.2)
  std::vector<int> v;
  v.reserve(make_size);
  while (v.size() != size) {
    while (v.size() < make_size) v.push_back(dist(rng));
    std::sort(v.begin(), v.end());
    auto unique_end = std::unique(v.begin(), v.end());
    if (size < (size_t)std::distance(v.begin(), unique_end)) unique_end = std::next(v.begin(), size);
    v.erase(unique_end, v.end());
  }
  std::shuffle(v.begin(), v.end(), rng);
  std::copy(v.begin(), v.end(), out);
}

void WindowEstimator::seedRansac() {
  const Config &c = config();
  if (ransac_seeded_ && ransac_seed_used_ == c.ransac_seed) return;
  if (c.ransac_seed != 0) {
    ransac_rng_.seed(c.ransac_seed);
  } else {  // random_array.cc:12-19
    std::random_device rd;
    std::vector<std::uint_least32_t> v(10);
    std::generate(v.begin(), v.end(), std::ref(rd));
    std::seed_seq seq(v.begin(), v.end());
    ransac_rng_.seed(seq);
  }
  ransac_seeded_ = true, ransac_seed_used_ = c.ransac_seed;
}

int WindowEstimator::calibrateExtrinsicRotation() {  // estimator.cpp:142-159
  Config &c = config();
  status = LFVIO_OK;
  if (!refreshSpans(false)) return status != LFVIO_OK ? status : LFVIO_ERR_DEVICE;
  const LfvioPreintegration &pre = span(frame_count).pre;
  const Quaterniond delta_q(pre.delta_q[3], pre.delta_q[0], pre.delta_q[1], pre.delta_q[2]);
  LastTwoView &tv = last_two_view;
  const int N = tracks.corresponding(frame_count - 1, frame_count, &tv.bl, &tv.br);
  tv.called = false;
  tv.samples.clear(), tv.mask.assign((size_t)N, 0);
  Matrix3d Rc = Matrix3d::Identity();  // fewer than 9 matches (initial_ex_rotation.cpp:223, :286)
  if (N >= 9) {
    if (!lfvio_two_view || !device()) return LFVIO_ERR_DEVICE;  // no fallback: without the device entry the mode cannot run
    seedRansac();
    const int S = std::max(1, c.ransac_iterations);
    tv.samples.resize((size_t)S * 8);
    for (int k = 0; k < S; k++) drawSampleSet(ransac_rng_, N, &tv.samples[(size_t)8 * k]);
    LfvioTwoViewIn in;
    in.num_matches = N, in.bearing_l = tv.bl.data(), in.bearing_r = tv.br.data(), in.num_samples = S, in.samples = tv.samples.data();
    std::memset(&tv.out, 0, sizeof tv.out);
    const int rc = lfvio_two_view(gpu, &in, tv.mask.data(), &tv.out, nullptr, nullptr);
    two_view_calls++;
    tv.called = true;
    if (rc != LFVIO_OK) return rc;
    if (tv.out.status == 0)  // status 1 (no model; include/lfvio.h): Rc = I, as for too few matches
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rc(i, j) = tv.out.R_rel[3 * i + j];
  }
  Matrix3d calib_ric;
  if (exrot.push(Rc, delta_q, &calib_ric)) {
    ric = calib_ric;  // ric[0] = calib_ric; RIC[0] = calib_ric; ESTIMATE_EXTRINSIC = 1
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) c.ric[3 * i + j] = calib_ric(i, j);
    c.estimate_extrinsic = 1;
  }
  return LFVIO_OK;
}

void WindowEstimator::pushImage(double stamp, int n, const int *ids, const double *pts8) {  // estimator.cpp:122-220
  marg_flag = keyframeTest(frame_count, n, ids, pts8, td) ? LFVIO_MARGIN_OLD : LFVIO_MARGIN_SECOND_NEW;
  kf(frame_count).stamp = stamp;
  {  // estimator.cpp:137-140: the image takes tmp_pre_integration, a new one starts at the last IMU sample with this frame's biases
    pending_.stamp = stamp;
    {  // :134 ImageFrame(image, header): the points, in the order of the reference's map
      std::vector<int> order(n);
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
      pending_.ids.resize(n), pending_.pts.resize(3 * (size_t)n);
      for (int k = 0; k < n; k++) {
        pending_.ids[k] = ids[order[k]];
        std::memcpy(&pending_.pts[3 * (size_t)k], pts8 + 8 * (size_t)order[k], 24);
      }
    }
    image_frames.push_back(std::move(pending_));
    pending_ = ImageFrame();
    const Keyframe &f = kf(frame_count);
    for (int k = 0; k < 3; k++) pending_.acc0[k] = acc_prev(k), pending_.gyr0[k] = gyr_prev(k), pending_.lin_ba[k] = f.Ba(k), pending_.lin_bg[k] = f.Bg(k);
  }
  if (config().estimate_extrinsic == 2 && frame_count != 0) {
    const int calib = calibrateExtrinsicRotation();
    advanceWindow(stamp);
    if (calib != LFVIO_OK) status = calib;
    return;
  }
  advanceWindow(stamp);
}

void WindowEstimator::advanceWindow(double stamp) {  // estimator.cpp:161-220
  auto remember = [&] { last_R = kf(WINDOW_SIZE).R, last_P = kf(WINDOW_SIZE).P, last_R0 = kf(0).R, last_P0 = kf(0).P; };
  if (phase == INITIAL) {
    if (frame_count < WINDOW_SIZE) {
      frame_count++;
      return;
    }
    bool aligned = false;
    if (config().estimate_extrinsic != 2 && stamp - initial_timestamp > 0.1) {
      // a bootstrap record wins (every recording made before there were SfM records replays as it did; it stays valid until the
      // next reset()); otherwise the SfM result of this image goes through the alignment.  The SfM result described this image's
      // list: it is dropped whether or not it was used
      bool from_sfm = false;
      if (bootstrap.valid) {
        aligned = applyBootstrap();
      } else if (sfm.valid) {
        aligned = visualInitialAlign();
        from_sfm = aligned;
      } else if (structure.valid) {  // the PnP loop first, then the same path
        aligned = solvePnpFrames() && visualInitialAlign();
        from_sfm = aligned;
      } else if (relative.valid || (config().self_relative_pose && relativePose())) {
        // a record wins; without one and with Config::self_relative_pose, relativePose() on the device fills `relative` (false: no pair
        // passed and the window slides with the flag the parallax test set).  GlobalSFM::construct() first, then the same path; a failed
        // construct() slides MARGIN_OLD (:284)
        const bool built = constructSfm();
        if (!built) marg_flag = LFVIO_MARGIN_OLD;
        aligned = built && solvePnpFrames() && visualInitialAlign();
        from_sfm = aligned;
      }
      sfm.valid = false;
      structure.valid = false;
      relative.valid = false;
      if (from_sfm && stop_after_align) return;
      initial_timestamp = stamp;
    }
    if (!aligned) {
      slide();
      return;
    }
    phase = NON_LINEAR;
    triangulate();
    optimization();
    slide();
    tracks.dropFailed();
    remember();
    return;
  }
  if (frame_count == WINDOW_SIZE) {  // solveOdometry(), estimator.cpp:475-486
    triangulate();
    optimization();
  }
  if (diverged()) {
    failure_occur = true;
    reset();  // as shipped, clearState() ends with failure_occur = 0 (estimator.cpp:82), so the flag does not survive the reboot
    return;
  }
  slide();
  tracks.dropFailed();
  remember();
}

bool WindowEstimator::diverged() const {  // estimator.cpp:628-674 as shipped: the other tests only log
  const Keyframe &f = kf(WINDOW_SIZE);
  if (f.Bg.norm() > 1.0) return true;
  if ((f.P - last_P).norm() > 5) return true;
  return std::abs(f.P.z() - last_P.z()) > 1;
}

void WindowEstimator::slide() {  // estimator.cpp:1011-1131
  if (frame_count != WINDOW_SIZE) return;
  Keyframe &newest = kf(WINDOW_SIZE);
  if (marg_flag == LFVIO_MARGIN_OLD) {
    const Matrix3d old_R = kf(0).R;
    const Vector3d old_P = kf(0).P;
    {  // estimator.cpp:1051-1067: everything up to and including Headers[0] leaves all_image_frame
      const double t_0 = kf(0).stamp;
      size_t keep = 0;
      while (keep < image_frames.size() && image_frames[keep].stamp <= t_0) keep++;
      image_frames.erase(image_frames.begin(), image_frames.begin() + keep);
    }
    // the ring turns: frame 1 becomes frame 0, ...; the slot of the old frame 0 becomes the new newest frame, which starts
    // as a copy of its predecessor with an empty span
    const Keyframe prev = newest;
    ring_.advance();
    kf(WINDOW_SIZE) = prev;
    span(WINDOW_SIZE).open(acc_prev, gyr_prev, prev.Ba, prev.Bg);
    slides_old++;
    if (phase == NON_LINEAR) {
      std::vector<TrackTable::Shifted> moved;
      tracks.dropOldestFrame(&moved);
      reanchorDepths(old_R * ric, old_P + old_R * tic, kf(0).R * ric, kf(0).P + kf(0).R * tic, moved);
    } else {
      tracks.dropOldestFrame(nullptr);
    }
    return;
  }
  // MARGIN_SECOND_NEW: the newest frame replaces the one before it, whose span takes the newest span's samples as well
  ImuSpan &keep = span(WINDOW_SIZE - 1), &gone = span(WINDOW_SIZE);
  for (int k = 0; k < gone.samples(); k++) keep.push(gone.dt[k], &gone.acc[3 * k], &gone.gyr[3 * k]);
  const double stamp = newest.stamp;
  kf(WINDOW_SIZE - 1) = newest;
  kf(WINDOW_SIZE - 1).stamp = stamp;
  gone.open(acc_prev, gyr_prev, newest.Ba, newest.Bg);
  slides_new++;
  tracks.dropSecondNewestFrame(frame_count);
}

void WindowEstimator::triangulate() {  // feature_manager.cpp:199-253: the 2k x 4 SVD per landmark runs on the device
  Stopwatch sw(&timers[2]);
  Staging &st = stage_;
  st.start_frame.clear(), st.obs_offset.assign(1, 0), st.point.clear(), st.lam_out.clear();
  std::vector<int> sel;
  for (int s : tracks.order()) {
    if (!tracks.solvable(s) || tracks.depth(s) > 0) continue;
    sel.push_back(s);
    st.start_frame.push_back(tracks.start(s));
    for (int k = 0; k < tracks.count(s); k++) {
      const double *o = tracks.obs(s, k);
      st.point.insert(st.point.end(), o, o + 3);
    }
    st.obs_offset.push_back((int)st.point.size() / 3);
    st.lam_out.push_back(tracks.depth(s));
  }
  if (sel.empty() || !device()) return;
  LfvioTriangulateIn in;
  in.num_landmarks = (int)sel.size(), in.num_observations = (int)st.point.size() / 3;
  in.start_frame = st.start_frame.data(), in.obs_offset = st.obs_offset.data(), in.obs_point = st.point.data();
  for (int f = 0; f < FRAMES; f++)
    for (int i = 0; i < 3; i++) {
      in.Ps[f][i] = kf(f).P(i);
      for (int j = 0; j < 3; j++) in.Rs[f][3 * i + j] = kf(f).R(i, j);
    }
  for (int i = 0; i < 3; i++) {
    in.tic[i] = tic(i);
    for (int j = 0; j < 3; j++) in.ric[3 * i + j] = ric(i, j);
  }
  in.init_depth = config().init_depth;
  status = lfvio_triangulate(gpu, &in, st.lam_out.data());
  if (status != LFVIO_OK) return;
  for (size_t k = 0; k < sel.size(); k++) tracks.setDepth(sel[k], st.lam_out[k]);
}

void WindowEstimator::reanchorDepths(const Matrix3d &old_R, const Vector3d &old_P, const Matrix3d &new_R, const Vector3d &new_P,
                                     const std::vector<TrackTable::Shifted> &moved) {  // feature_manager.cpp:291-299
  Stopwatch sw(&timers[3]);
  if (moved.empty() || !device()) return;
  std::vector<double> uv(3 * moved.size()), depth(moved.size());
  for (size_t k = 0; k < moved.size(); k++) {
    std::memcpy(&uv[3 * k], moved[k].bearing, 3 * sizeof(double));
    depth[k] = tracks.depth(moved[k].slot);
  }
  double mR[9], nR[9], mP[3], nP[3];
  for (int i = 0; i < 3; i++) {
    mP[i] = old_P(i), nP[i] = new_P(i);
    for (int j = 0; j < 3; j++) mR[3 * i + j] = old_R(i, j), nR[3 * i + j] = new_R(i, j);
  }
  status = lfvio_shift_depth(gpu, (int)moved.size(), uv.data(), mR, mP, nR, nP, config().init_depth, depth.data());
  if (status != LFVIO_OK) return;
  for (size_t k = 0; k < moved.size(); k++) tracks.setDepth(moved[k].slot, depth[k]);
}

bool WindowEstimator::refreshSpans(bool all, const Vector3d *ba, const Vector3d *bg) {
  Stopwatch sw(&timers[4]);
  // IntegrationBase::{push_back, propagate, repropagate} (integration_base.h:29-158) for every span whose samples or
  // linearization biases changed since its `pre` was made — all of them in ONE device call
  std::vector<LfvioImuInterval> in;
  std::vector<int> which;
  for (int i = 0; i < FRAMES; i++) {
    ImuSpan &sp = span(i);
    if (!sp.present) continue;
    if (ba)
      for (int k = 0; k < 3; k++) sp.lin_ba[k] = ba[i](k), sp.lin_bg[k] = bg[i](k);
    if (!(all || sp.dirty)) continue;
    LfvioImuInterval iv;
    iv.num_samples = sp.samples();
    iv.dt = sp.dt.data(), iv.acc = sp.acc.data(), iv.gyr = sp.gyr.data();
    std::memcpy(iv.acc_0, sp.acc0, sizeof iv.acc_0), std::memcpy(iv.gyr_0, sp.gyr0, sizeof iv.gyr_0);
    std::memcpy(iv.linearized_ba, sp.lin_ba, sizeof iv.linearized_ba), std::memcpy(iv.linearized_bg, sp.lin_bg, sizeof iv.linearized_bg);
    in.push_back(iv), which.push_back(i);
  }
  if (in.empty()) return true;
  if (!device()) return false;
  std::vector<LfvioPreintegration> out(in.size());
  const Config &c = config();
  const double noise[4] = {c.acc_n, c.gyr_n, c.acc_w, c.gyr_w};
  status = lfvio_preintegrate(gpu, (int)in.size(), in.data(), noise, out.data());
  if (status != LFVIO_OK) return false;
  for (size_t k = 0; k < in.size(); k++) {
    ImuSpan &sp = span(which[k]);
    sp.pre = out[k];
    sp.sum_dt = out[k].sum_dt;
    sp.dirty = false;
  }
  return true;
}

void WindowEstimator::vector2double() {  // estimator.cpp:488-530
  for (int i = 0; i < FRAMES; i++) {
    const Keyframe &f = kf(i);
    const Quaterniond q{f.R};
    const double pose[7] = {f.P.x(), f.P.y(), f.P.z(), q.x(), q.y(), q.z(), q.w()};
    const double sb[9] = {f.V.x(), f.V.y(), f.V.z(), f.Ba.x(), f.Ba.y(), f.Ba.z(), f.Bg.x(), f.Bg.y(), f.Bg.z()};
    std::memcpy(para_Pose[i], pose, sizeof pose);
    std::memcpy(para_SpeedBias[i], sb, sizeof sb);
  }
  const Quaterniond qe{ric};
  const double ex[7] = {tic.x(), tic.y(), tic.z(), qe.x(), qe.y(), qe.z(), qe.w()};
  std::memcpy(para_Ex_Pose[0], ex, sizeof ex);
  para_Feature.clear();
  for (int s : tracks.order())
    if (tracks.solvable(s)) para_Feature.push_back(1. / tracks.depth(s));  // getDepthVector(), feature_manager.cpp:181-197
  if (config().estimate_td) para_Td[0][0] = td;
}

void WindowEstimator::double2vector() {  // estimator.cpp:532-600, and the relocalization tail :603-625
  Vector3d origin_R0 = yawPitchRollDeg(kf(0).R);
  Vector3d origin_P0 = kf(0).P;
  if (failure_occur) {
    origin_R0 = yawPitchRollDeg(last_R0);
    origin_P0 = last_P0;
    failure_occur = false;
  }
  auto quat = [](const double *p) { return Quaterniond(p[6], p[3], p[4], p[5]); };
  const Vector3d origin_R00 = yawPitchRollDeg(quat(para_Pose[0]).toRotationMatrix());
  const double y_diff = origin_R0.x() - origin_R00.x();
  Matrix3d rot_diff = fromYawPitchRollDeg(Vector3d(y_diff, 0, 0));
  if (std::abs(std::abs(origin_R0.y()) - 90) < 1.0 || std::abs(std::abs(origin_R00.y()) - 90) < 1.0)
    rot_diff = kf(0).R * quat(para_Pose[0]).toRotationMatrix().transpose();  // singular pitch
  for (int i = 0; i < FRAMES; i++) {
    Keyframe &f = kf(i);
    const double *p = para_Pose[i], *s = para_SpeedBias[i];
    f.R = rot_diff * quat(p).normalized().toRotationMatrix();
    f.P = rot_diff * Vector3d(p[0] - para_Pose[0][0], p[1] - para_Pose[0][1], p[2] - para_Pose[0][2]) + origin_P0;
    f.V = rot_diff * Vector3d(s[0], s[1], s[2]);
    f.Ba = Vector3d(s[3], s[4], s[5]);
    f.Bg = Vector3d(s[6], s[7], s[8]);
  }
  tic = Vector3d(para_Ex_Pose[0][0], para_Ex_Pose[0][1], para_Ex_Pose[0][2]);
  ric = quat(para_Ex_Pose[0]).toRotationMatrix();
  size_t k = 0;
  for (int s : tracks.order()) {
    if (!tracks.solvable(s)) continue;
    tracks.setDepth(s, 1.0 / para_Feature[k++]);  // setDepth(), feature_manager.cpp:139-156
    tracks.setSolveFlag(s, 1);                     // both branches of the reference set 1
  }
  if (config().estimate_td) td = para_Td[0][0];
  if (relocalization_info) {  // relative info between two loop frames, estimator.cpp:603-625
    const Matrix3d relo_r = rot_diff * quat(relo_Pose).normalized().toRotationMatrix();
    const Vector3d relo_t =
        rot_diff * Vector3d(relo_Pose[0] - para_Pose[0][0], relo_Pose[1] - para_Pose[0][1], relo_Pose[2] - para_Pose[0][2]) + origin_P0;
    const double drift_correct_yaw = yawPitchRollDeg(prev_relo_r).x() - yawPitchRollDeg(relo_r).x();
    drift_correct_r = fromYawPitchRollDeg(Vector3d(drift_correct_yaw, 0, 0));
    drift_correct_t = prev_relo_t - drift_correct_r * relo_t;
    const Keyframe &f = kf(relo_frame_local_index);
    relo_relative_t = relo_r.transpose() * (f.P - relo_t);
    relo_relative_q = Quaterniond(relo_r.transpose() * f.R);
    double a = yawPitchRollDeg(f.R).x() - yawPitchRollDeg(relo_r).x();  // Utility::normalizeAngle
    a = a > 0 ? a - 360.0 * std::floor((a + 180.0) / 360.0) : a + 360.0 * std::floor((-a + 180.0) / 360.0);
    relo_relative_yaw = a;
    relocalization_info = 0;
  }
}

// estimator.cpp:1133-1151, literally: the relo pose starts from para_Pose[i] AS IT STANDS — after a slide that is the row of the
// frame that was at i BEFORE the slide (slideWindow() shifts Ps / Rs, not para_Pose; vector2double() refreshes it only in the next
// optimization()).  It is only the initial value of relo_Pose, but an iteration-capped solve ends elsewhere with another one.
void WindowEstimator::setReloFrame(double stamp, int index, const std::vector<Vector3d> &points, const Vector3d &relo_t, const Matrix3d &relo_r) {
  relo_frame_stamp = stamp;
  relo_frame_index = index;
  match_points = points;
  prev_relo_t = relo_t;
  prev_relo_r = relo_r;
  for (int i = 0; i < WINDOW_SIZE; i++) {
    if (relo_frame_stamp == kf(i).stamp) {
      relo_frame_local_index = i;
      relocalization_info = 1;
      for (int j = 0; j < LFVIO_SIZE_POSE; j++) relo_Pose[j] = para_Pose[i][j];
    }
  }
}

int WindowEstimator::reloMatches(std::vector<int> *landmark, std::vector<double> *xy) const {
  landmark->clear(), xy->clear();
  const size_t K = match_points.size();
  size_t k = 0;
  int l = -1;
  for (int s : tracks.order()) {
    if (!tracks.solvable(s)) continue;
    ++l;
    if (tracks.start(s) > relo_frame_local_index) continue;
    while (k < K && (int)match_points[k].z() < tracks.id(s)) k++;
    if (k < K && (int)match_points[k].z() == tracks.id(s)) {
      landmark->push_back(l);
      xy->push_back(match_points[k].x()), xy->push_back(match_points[k].y());
      k++;
    }
  }
  return (int)landmark->size();
}

void WindowEstimator::pack(LfvioWindow *w) {
  const Config &c = config();
  if (!chain_upload_) (void)collectPrior();  // (optimization() on one device lets the upload collect it: lfvio_batch_upload_chained)
  std::memset(w, 0, sizeof *w);
  std::memcpy(w->para_pose, para_Pose, sizeof para_Pose);
  std::memcpy(w->para_speed_bias, para_SpeedBias, sizeof para_SpeedBias);
  std::memcpy(w->para_ex_pose, para_Ex_Pose[0], sizeof para_Ex_Pose[0]);
  w->para_td = c.estimate_td ? para_Td[0][0] : td;
  w->estimate_extrinsic = c.estimate_extrinsic != 0;
  w->estimate_td = c.estimate_td != 0;
  w->max_num_iterations = c.num_iterations;
  // estimator.cpp:819-822; <= 0 disables the cap (parity / bench)
  w->max_solver_time_in_seconds = c.solver_time <= 0 ? -1.0 : (marg_flag == LFVIO_MARGIN_OLD ? c.solver_time * 4.0 / 5.0 : c.solver_time);
  std::memcpy(w->g, c.gravity, sizeof w->g);
  w->tr = c.tr, w->row = c.row;
  w->sqrt_info = FOCAL_LENGTH / 1.5;  // estimator.cpp:18-19
  // the solvable tracks in table order -> CSR: one pass, sized once
  Staging &st = stage_;
  const int N = tracks.solvableCount();
  int M = 0;
  for (int s : tracks.order())
    if (tracks.solvable(s)) M += tracks.count(s);
  st.start_frame.resize(N), st.obs_offset.resize(N + 1), st.inv_depth.resize(N);
  st.point.resize(3 * (size_t)M), st.velocity.resize(3 * (size_t)M), st.cur_td.resize(M), st.uv_y.resize(M);
  int l = 0, o = 0;
  st.obs_offset[0] = 0;
  for (int s : tracks.order()) {
    if (!tracks.solvable(s)) continue;
    st.start_frame[l] = tracks.start(s);
    st.inv_depth[l] = para_Feature[l];
    for (int k = 0; k < tracks.count(s); k++, o++) {
      const double *r = tracks.obs(s, k);
      std::memcpy(&st.point[3 * (size_t)o], r, 3 * sizeof(double));
      std::memcpy(&st.velocity[3 * (size_t)o], r + 5, 3 * sizeof(double));
      st.uv_y[o] = r[4];
      st.cur_td[o] = r[8];
    }
    st.obs_offset[++l] = o;
  }
  w->num_landmarks = N, w->num_observations = M;
  w->start_frame = st.start_frame.data(), w->obs_offset = st.obs_offset.data(), w->inv_depth = st.inv_depth.data();
  w->obs_point = st.point.data(), w->obs_velocity = st.velocity.data(), w->obs_cur_td = st.cur_td.data(), w->obs_uv_y = st.uv_y.data();
  for (int i = 0; i < WINDOW_SIZE; i++) {  // pre_integrations[1..10] (estimator.cpp:717-724)
    const ImuSpan &sp = span(i + 1);
    if (sp.present) w->imu[i] = sp.pre;
    else w->imu[i].sum_dt = 1e9;  // no factor
  }
  w->prior = has_prior ? &prior : nullptr;
}

// estimator.cpp:676-1009 over the C-ABI.  On any error the state is left as the caller had it — but for a prior that was lost on the
// device with the failed call, see below — and `status` says why (the
// reference has no error channel at all).
void WindowEstimator::optimization() {
  status = LFVIO_OK;
  if (!device() || !refreshSpans(false)) return;
  if (relocalization_info) {
    optimizationRelo();
    return;
  }
  // The marginalization behind the previous call's early state may still be running.  On one device with one upload the
  // window is packed and its tables are built while it finishes: the upload collects the prior itself (chained); every other
  // route waits for it here.
  const bool chain = prior_pending_ && fused && !group && config().split_call;
  if (!chain && !collectPrior()) return;
  Stopwatch sw(&timers[0]);
  timers[5] += 1.0;
  vector2double();  // :707
  LfvioWindow w;
  chain_upload_ = chain;
  pack(&w);
  chain_upload_ = false;
  Staging &st = stage_;
  st.lam_out.assign(w.num_landmarks > 0 ? w.num_landmarks : 1, 0.0);
  bool second_new = marg_flag == LFVIO_MARGIN_SECOND_NEW && has_prior && prior.valid;  // (chained upload: decided again once the prior is there)
  bool marginalize = marg_flag == LFVIO_MARGIN_OLD || second_new;
  auto take_state = [&] {
    std::memcpy(para_Pose, summary.para_pose, sizeof para_Pose);
    std::memcpy(para_SpeedBias, summary.para_speed_bias, sizeof para_SpeedBias);
    std::memcpy(para_Ex_Pose[0], summary.para_ex_pose, sizeof para_Ex_Pose[0]);
    if (config().estimate_td) para_Td[0][0] = summary.para_td;
    std::copy(st.lam_out.begin(), st.lam_out.begin() + w.num_landmarks, para_Feature.begin());
    double2vector();  // :830
  };
  LfvioPrior &next = next_;
  summary.inv_depth = st.lam_out.data();
  if (group) {
    // several devices: the same three steps as below in ONE call — the landmarks sharded over the devices of the group,
    // every collective an ncclAllReduce the library issues itself (lf-vio_amd/csrc/group.inc)
    status = lfvio_group_solve(group, &w, marg_flag, &summary, &next);
    summary.inv_depth = nullptr;
    if (status != LFVIO_OK) return;
    take_state();
    if (marginalize) assign_prior(&prior, &next), has_prior = next.valid != 0;
    return;
  }
  if (fused) {
    // one upload; solve (:810-825), the gauge fix of double2vector() (:532-626) and the marginalization (:833-1005) run back
    // to back on the device.  The state that comes back is already re-anchored, so double2vector() below applies a zero
    // yaw and a zero shift to it.
    status = lfvio_batch_reserve(gpu, 1, w.num_landmarks, w.num_observations);
    if (status == LFVIO_OK && chain) {
      // `prior` is an output here first (the prior of the call in flight), then the window's input
      w.prior = nullptr;
      // first choice: the prior stays on the device and nothing is waited for.  Refused with LFVIO_ERR_ARG — and the call in flight
      // untouched — when that marginalization passes its input prior through or the window is malformed: the host-side hand-over
      // then decides (it reports a malformed window itself).
      status = config().device_chain ? lfvio_batch_upload_chained_device(gpu, 0, &w) : LFVIO_ERR_ARG;
      if (status == LFVIO_OK) {
        // the window's prior is on the device only; the host's copy `prior` is the one of two windows back from here on, until the
        // next marginalization is collected
        prior_pending_ = false, has_prior = true, prior_on_device_ = true;
      } else {
        status = lfvio_batch_upload_chained(gpu, 0, &w, &prior);
        prior_pending_ = lfvio_batch_optimize_pending(gpu) != 0;  // (an upload refused before it got to the prior leaves it where it was)
        if (!prior_pending_) has_prior = prior.valid != 0;
      }
      if (status == LFVIO_OK) {
        second_new = marg_flag == LFVIO_MARGIN_SECOND_NEW && has_prior;
        marginalize = marg_flag == LFVIO_MARGIN_OLD || second_new;
      }
    } else if (status == LFVIO_OK)
      status = lfvio_batch_upload(gpu, 0, &w);
    if (status == LFVIO_OK && config().split_call) {
      // The state comes back as soon as solve + gauge fix are out (the device pushes it into mapped host memory); the
      // marginalization runs on while the caller publishes the pose, slides the window, takes the next image — its prior is
      // collected by the first thing that needs it (collectPrior(): the next pack()).
      status = lfvio_batch_optimize_begin(gpu, marg_flag, &summary);
      summary.inv_depth = nullptr;
      if (status != LFVIO_OK) {
        // A window that took its prior over on the device and did not get through (the prior was not there, a device error): that
        // prior is gone with the call, and the host's copy is two windows old — its frames have been shifted twice since.  The
        // estimator goes on WITHOUT a prior rather than with that one.
        if (prior_on_device_) has_prior = false, prior.valid = 0, prior_on_device_ = false;
        return;
      }
      take_state();
      if (marginalize) prior_pending_ = true;
      else (void)lfvio_batch_optimize_finish(gpu, nullptr);
      if (marginalize) prior_on_device_ = false;  // (what is collected next is this call's own prior)
      return;
    }
    if (status == LFVIO_OK) status = lfvio_batch_optimize(gpu, 1, marg_flag);
    if (status == LFVIO_OK) status = lfvio_batch_download(gpu, 0, &summary, marginalize ? &next : nullptr);
    summary.inv_depth = nullptr;
    if (status != LFVIO_OK) return;
    take_state();
    if (marginalize) assign_prior(&prior, &next), has_prior = next.valid != 0;
    return;
  }
  // the reference's literal sequence: solve, double2vector() on the host, vector2double(), marginalize (two uploads)
  status = lfvio_solve(gpu, &w, &summary);
  summary.inv_depth = nullptr;
  if (status != LFVIO_OK) return;
  take_state();
  if (!marginalize) return;
  vector2double();
  pack(&w);
  status = lfvio_marginalize(gpu, &w, marg_flag, &next);
  if (status != LFVIO_OK) return;
  assign_prior(&prior, &next), has_prior = next.valid != 0;
}

// The relocalization branch (estimator.cpp:777-808) in the reference's two-call form on the first context (of the group, if any):
// the prior of the last call is collected first, then lfvio_solve_relo, double2vector() with its relo tail, vector2double() and
// lfvio_marginalize.  The next window goes back to the configured route: nothing of this call stays in flight.
void WindowEstimator::optimizationRelo() {
  if (!collectPrior()) return;
  Stopwatch sw(&timers[0]);
  timers[5] += 1.0;
  vector2double();
  LfvioWindow w;
  pack(&w);
  Staging &st = stage_;
  st.lam_out.assign(w.num_landmarks > 0 ? w.num_landmarks : 1, 0.0);
  const int K = reloMatches(&relo_lm_, &relo_xy_);
  LfvioRelo r;
  r.frame = relo_frame_local_index;
  std::memcpy(r.relo_pose, relo_Pose, sizeof r.relo_pose);
  r.num_matches = K;
  r.landmark = K ? relo_lm_.data() : nullptr;
  r.match_point = K ? relo_xy_.data() : nullptr;
  const bool marginalize = marg_flag == LFVIO_MARGIN_OLD || (marg_flag == LFVIO_MARGIN_SECOND_NEW && has_prior && prior.valid);
  double relo_out[LFVIO_SIZE_POSE];
  if (!lfvio_solve_relo) {
    status = LFVIO_ERR_DEVICE;
    return;
  }
  summary.inv_depth = st.lam_out.data();
  status = lfvio_solve_relo(gpu, &w, &r, &summary, relo_out);
  summary.inv_depth = nullptr;
  if (status != LFVIO_OK) return;
  std::memcpy(para_Pose, summary.para_pose, sizeof para_Pose);
  std::memcpy(para_SpeedBias, summary.para_speed_bias, sizeof para_SpeedBias);
  std::memcpy(para_Ex_Pose[0], summary.para_ex_pose, sizeof para_Ex_Pose[0]);
  if (config().estimate_td) para_Td[0][0] = summary.para_td;
  std::copy(st.lam_out.begin(), st.lam_out.begin() + w.num_landmarks, para_Feature.begin());
  std::memcpy(relo_Pose, relo_out, sizeof relo_Pose);
  double2vector();  // :830, with the relo tail; clears relocalization_info
  relo_solves++;
  if (!marginalize) return;
  vector2double();
  pack(&w);
  status = lfvio_marginalize(gpu, &w, marg_flag, &next_);
  if (status != LFVIO_OK) return;
  assign_prior(&prior, &next_), has_prior = next_.valid != 0;
}

}  // namespace lfvio
