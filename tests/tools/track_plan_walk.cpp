// track_plan_walk.cpp — a stand-alone walk over the argument checks of lf-vio_amd/csrc/track_plan.h for a sanitizer build of the
// host side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc tests/tools/track_plan_walk.cpp -o track_plan_walk
//   ./track_plan_walk
// Every array is allocated at exactly the size the call declares, so a check that reads past num_points, 8 * num_samples or the
// camera is an error the sanitizer reports.  Prints the number of accepted and refused combinations; exit code 1 when a verdict is
// not the expected one.
#include <cstdio>
#include <limits>
#include <vector>

#include "track_plan.h"

static int bad = 0, accepted = 0, refused = 0;

static void expect(const char *why, bool want_refused, const char *what) {
  if ((why != nullptr) != want_refused) std::printf("WRONG: %s -> %s\n", what, why ? why : "accepted"), bad++;
  (why ? refused : accepted)++;
}

int main() {
  LfvioCamera cam = {LFVIO_CAM_OCAM, 645.1, 486.0, 1.0, 0.0, 0.0, {-244.5, 0.0, 1.7e-3, -1.8e-6, 4.5e-9}};
  LfvioCamera other = cam;
  other.model = 1;
  const TrackCam t = track_cam(cam);
  if (t.inv_scale != 1.0) std::printf("WRONG: inv_scale\n"), bad++;
  const int sizes[] = {-1, 0, 1, 7, 8, 9, 64, 4096, 4097};
  const int counts[] = {-1, 0, 1, 100, 1024, 1025};
  for (int N : sizes) {
    const size_t n = N > 0 && N <= LFVIO_TRACK_MAX_POINTS ? (size_t)N : 0;
    std::vector<float> cur(2 * n, 10.0f), forw(2 * n, 11.0f);
    std::vector<int> ids(n, 3);
    const bool n_ok = N >= 0 && N <= LFVIO_TRACK_MAX_POINTS;
    for (int S : counts) {
      const size_t s = S > 0 && S <= TRACK_MAX_SAMPLES ? (size_t)S : 0;
      std::vector<int> samples(8 * s);
      for (size_t k = 0; k < samples.size(); k++) samples[k] = n ? (int)(k % n) : 0;
      const bool runs = n_ok && N >= TRACK_MIN_MATCHES, s_ok = S >= 1 && S <= TRACK_MAX_SAMPLES;
      LfvioTrackRejectIn in = {&cam, N, n ? cur.data() : nullptr, n ? forw.data() : nullptr, S, s ? samples.data() : nullptr};
      expect(track_reject_check(&in), !n_ok || (runs && !s_ok), "reject: sizes");
      if (runs && s_ok) {
        samples.back() = N;
        expect(track_reject_check(&in), true, "reject: sample index N");
        samples.back() = -1;
        expect(track_reject_check(&in), true, "reject: sample index -1");
        samples.back() = N - 1;
        expect(track_reject_check(&in), false, "reject: sample index N - 1");
        in.samples = nullptr;
        expect(track_reject_check(&in), true, "reject: null samples");
        in.samples = samples.data();
      }
      in.camera = nullptr;
      expect(track_reject_check(&in), true, "reject: null camera");
      in.camera = &other;
      expect(track_reject_check(&in), true, "reject: model");
      in.camera = &cam;
      if (n_ok && N > 0) {
        in.cur_pts = nullptr;
        expect(track_reject_check(&in), true, "reject: null cur_pts");
        in.cur_pts = cur.data(), in.forw_pts = nullptr;
        expect(track_reject_check(&in), true, "reject: null forw_pts");
      }
    }
    const double times[] = {0.0, -3.5, 1e300, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (double time : times) {
      LfvioTrackUndistortIn in = {&cam, N, n ? cur.data() : nullptr, n ? ids.data() : nullptr, time};
      expect(track_undistort_check(&in), !n_ok || time != time, "undistort: sizes and time");
      in.camera = &other;
      expect(track_undistort_check(&in), true, "undistort: model");
      in.camera = nullptr;
      expect(track_undistort_check(&in), true, "undistort: null camera");
      in.camera = &cam;
      if (n_ok && N > 0) {
        in.pts = nullptr;
        expect(track_undistort_check(&in), true, "undistort: null pts");
        in.pts = cur.data(), in.ids = nullptr;
        expect(track_undistort_check(&in), true, "undistort: null ids");
      }
    }
  }
  std::printf("track_plan walk: %d accepted, %d refused, %d wrong\n", accepted, refused, bad);
  return bad ? 1 : 0;
}
