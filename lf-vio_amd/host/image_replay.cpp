// image_replay.cpp — see image_replay.h.
#include "image_replay.h"

#include <chrono>
#include <cstdio>
#include <cstring>

namespace lfvio {

namespace {
void put(std::vector<char> *out, const void *p, size_t n) {
  const char *c = (const char *)p;
  out->insert(out->end(), c, c + n);
}
void record(std::vector<char> *out, uint32_t type, const void *a, size_t na, const void *b = nullptr, size_t nb = 0) {
  const uint32_t head[2] = {type, (uint32_t)(na + nb)};
  put(out, head, sizeof head);
  put(out, a, na);
  if (nb) put(out, b, nb);
}
}  // namespace

int trackRecording(FeatureTracker &tracker, const char *in_path, std::vector<char> *out, TrackStats *stats) {
  TrackStats st;
  std::memset(&st, 0, sizeof st);
  auto finish = [&](int rc) {
    if (stats) *stats = st;
    return rc;
  };
  {
    Trace check;  // every refusal of the loader is this call's: the pass below trusts the lengths
    if (!check.load(in_path)) return finish(-3);
  }
  std::FILE *f = std::fopen(in_path, "rb");
  if (!f) return finish(-3);
  char file_head[8];
  if (std::fread(file_head, 1, 8, f) != 8) {
    std::fclose(f);
    return finish(-3);
  }
  out->clear();
  put(out, file_head, 8);
  std::vector<char> buf;
  TraceImage msg;
  int rc = 0;
  for (;;) {
    uint32_t head[2];
    if (std::fread(head, 4, 2, f) != 2) break;
    buf.resize(head[1]);
    if (head[1] && std::fread(buf.data(), 1, head[1], f) != head[1]) {
      rc = -3;
      break;
    }
    if (head[0] != 10) {
      record(out, head[0], buf.data(), buf.size());
      continue;
    }
    double stamp;
    uint32_t dims[4];  // width, height, step, encoding
    std::memcpy(&stamp, buf.data(), 8), std::memcpy(dims, buf.data() + 8, 16);
    st.raw_images++;
    const auto t0 = std::chrono::steady_clock::now();
    const int what = tracker.onImage(stamp, (int)dims[0], (int)dims[1], (int)dims[2], (int)dims[3], (const unsigned char *)buf.data() + 24, &msg);
    st.tracker_ms += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    if (what < 0) {  // a device call failed: no silent continuation
      rc = -2;
      break;
    }
    switch (what) {
      case FeatureTracker::DROPPED:
        st.dropped++;
        break;
      case FeatureTracker::RESTART:  // std_msgs/Bool(true) on the restart topic (feature_tracker_node.cpp:44-46)
        st.restarts++;
        record(out, 5, &stamp, 8);
        break;
      case FeatureTracker::PUBLISHED: {
        st.published++, st.rows += (double)msg.size();
        struct {
          double t;
          uint32_t n;
        } __attribute__((packed)) mh = {msg.t, (uint32_t)msg.size()};
        static_assert(sizeof mh == 12, "packed");
        record(out, 2, &mh, sizeof mh, msg.v.data(), msg.v.size() * sizeof(float));
        break;
      }
      default:  // tracked only, or the first publication, which the node skips
        st.tracked_only++;
    }
  }
  std::fclose(f);
  return finish(rc);
}

int trackTrace(FeatureTracker &tracker, const char *in_path, const char *out_path, TrackStats *stats) {
  std::vector<char> bytes;
  if (int rc = trackRecording(tracker, in_path, &bytes, stats)) return rc;
  std::FILE *f = std::fopen(out_path, "wb");
  if (!f) return -1;
  const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  return std::fclose(f) == 0 && ok ? 0 : -1;
}

int replayImages(WindowEstimator &estimator, FeatureTracker &tracker, const char *path, const char *traj_path, int max_images, ReplayStats *stats,
                 TrackStats *track_stats, std::vector<double> *image_ms) {
  if (stats) std::memset(stats, 0, sizeof *stats);
  std::vector<char> bytes;
  if (int rc = trackRecording(tracker, path, &bytes, track_stats)) {
    if (stats && rc == -2) stats->last_status = tracker.status;
    return rc;
  }
  std::FILE *f = fmemopen(bytes.data(), bytes.size(), "rb");
  if (!f) return -3;
  Trace trace;
  const bool ok = trace.read(f);
  std::fclose(f);
  if (!ok) return -3;
  return replay(estimator, trace, traj_path, max_images, stats, image_ms);
}

}  // namespace lfvio
