// track_node_walk.cpp — a stand-alone walk over lf-vio_amd/host/track_node.h and trace_rewrite.{h,cpp} for a sanitizer build of the host
// side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -ffunction-sections -Wl,--gc-sections
//       -I lf-vio_amd/host tests/tools/track_node_walk.cpp lf-vio_amd/host/trace_rewrite.cpp lf-vio_amd/host/replay.cpp
//       -o track_node_walk                                                                                  (one line)
//   ./track_node_walk a.lfvt b.lfvt ...          (recordings with raw images, e.g. lfvio.trace.make_image_stream's)
// (replay.cpp for Trace::load; its replay(), which drives the estimator, is not referenced and leaves with its section.)
// The recordings go through rewriteRecordings together and each alone, the round a tracker node WITHOUT a device: every stream's
// ImageGate, NodeSettings::apply against a route that counts its calls, FrameBuffers::fill with the stream's generator, then — in the
// device call's place — every byte of the image read (height rows of step bytes, exactly the record's: a read behind it is the
// sanitizer's to report) and two rows written into the arrays that fill bound, frameResult and FrameBuffers::message.  Checked: a
// recording alone gives the bytes and counts it gives among the others, every output is a well-formed file without raw images whose
// type-2 and type-5 records are as many as the counts say, the settings were made once per walk, a round that fails gives -2 with
// its images counted, a missing file gives -3.  Exit code 1 when something is not as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "trace_rewrite.h"
#include "track_node.h"

using namespace lfvio;

static int bad = 0;
static void wrong(const char *what) { std::printf("WRONG: %s\n", what), bad++; }

struct Counting final : SettingsRoute {
  int calls[5] = {0, 0, 0, 0, 0};
  long mask_sum = 0;
  int mask(int w, int h, const unsigned char *p) override {
    for (long k = 0; p && k < (long)w * h; k++) mask_sum += p[k];
    return calls[0]++, 0;
  }
  int clahe(const LfvioClaheIn *c) override { return calls[1] += c && c->tiles_x == 8, 0; }
  int format(const LfvioImageFormat *) override { return calls[2]++, 0; }
  int map(const LfvioRemapIn *in) override { return calls[3] += in->proj->camera->cx == 3.5 && in->width == 64, 0; }
  int source(const LfvioTrackSource *) override { return calls[4]++, 0; }
};

// n tracker nodes without a device
struct Node {
  TrackerConfig cfg;
  NodeSettings settings;
  Counting route;
  std::vector<ImageGate> gate;
  std::vector<std::mt19937> rng;
  std::vector<FrameBuffers> buffers;
  long bytes_read = 0, words_drawn = 0;
  int fail_round = -1, round = 0;
  explicit Node(int n, bool expand) : gate((size_t)n), rng((size_t)n), buffers((size_t)n) {
    cfg.equalize = true, cfg.annulus = true, cfg.center_x = 31.5, cfg.center_y = 23.25, cfg.max_r = 20.0, cfg.min_r = 6.0;
    cfg.num_samples = 7, cfg.ransac_seed = 77;
    if (expand) cfg.expand.on = true, cfg.expand.width = 64, cfg.expand.height = 32, cfg.expand.src_camera.cx = 3.5;
    for (std::mt19937 &r : rng) seedSamples(r, cfg.ransac_seed);
  }
  int onRound(BatchEntry *entries) {
    if (round++ == fail_round) return -1;
    for (size_t i = 0; i < gate.size(); i++) {
      BatchEntry &e = entries[i];
      if (!e.present) continue;
      if (imageArgsBad(e.width, e.height, e.step, e.encoding, e.pixels)) return -1;
      const ImageGate::Stamp what = gate[i].onStamp(e.stamp);
      if (what != ImageGate::TRACK) {
        e.result = what == ImageGate::DROP ? TrackResults::DROPPED : TrackResults::RESTART;
        continue;
      }
      if (int rc = settings.apply(cfg, e.width, e.height, {e.encoding, e.step}, route)) return rc;
      LfvioTrackFrameIn in;
      LfvioTrackFrameOut out;
      LfvioTrackMessage msg;
      buffers[i].fill(cfg, trackedWidth(cfg, e.width), trackedHeight(cfg, e.height), e.pixels, e.stamp, gate[i].publish, rng[i], &in, &out, &msg);
      if (in.win_size != 41 || in.capacity != LFVIO_TRACK_MAX_POINTS || (in.sample_words != nullptr) != gate[i].publish) wrong("the frame's arguments");
      unsigned sum = 0;  // the device call's place
      for (long b = 0; b < (long)e.height * e.step; b++) sum += in.image[b];
      bytes_read += (long)e.height * e.step;
      for (int k = 0; in.sample_words && k < 8 * in.num_samples; k++) sum += in.sample_words[k], words_drawn++;
      if (in.publish) {
        msg.num_rows = 2;
        for (int c = 0; c < 18; c++) msg.rows[c] = (float)(sum % 4096u) + (float)c;
        out.pts[2 * LFVIO_TRACK_MAX_POINTS - 1] = 1.0f, out.velocity_3d[3 * LFVIO_TRACK_MAX_POINTS - 1] = 1.0f, out.ids[LFVIO_TRACK_MAX_POINTS - 1] = 1;
        msg.rows[9 * LFVIO_TRACK_MAX_POINTS - 1] = 0.0f;  // the arrays' last entries are the caller's to write
      }
      e.result = frameResult(gate[i].afterFrame());
      if (e.result == TrackResults::PUBLISHED) buffers[i].message(e.stamp, msg.num_rows, &e.msg);
    }
    return 0;
  }
};

// the records of an output: well-formed, no raw image, and how many messages and restarts
static bool census(const std::vector<char> &body, long *messages, long *restarts) {
  *messages = *restarts = 0;
  if (body.size() < 8 || std::memcmp(body.data(), "LFVT", 4)) return false;
  size_t at = 8;
  while (at < body.size()) {
    uint32_t head[2];
    if (at + 8 > body.size()) return false;
    std::memcpy(head, body.data() + at, 8);
    if (at + 8 + head[1] > body.size() || head[0] == 10) return false;
    if (head[0] == 2) {
      uint32_t n;
      std::memcpy(&n, body.data() + at + 16, 4);
      if (head[1] != 12 + 36 * n) return false;  // the packed head and n rows of nine floats
      ++*messages;
    }
    if (head[0] == 5) {
      if (head[1] != 8) return false;
      ++*restarts;
    }
    at += 8 + head[1];
  }
  return true;
}

int main(int argc, char **argv) {
  const int n = argc - 1;
  if (n < 1) {
    std::printf("usage: track_node_walk recording...\n");
    return 1;
  }
  const char *const *paths = argv + 1;
  long published = 0, images = 0, bytes = 0;
  for (int expand = 0; expand < 2; expand++) {
    Node all(n, expand != 0);
    std::vector<std::vector<char>> outs;
    std::vector<TrackStats> st((size_t)n);
    if (rewriteRecordings(n, paths, &outs, st.data(), [&](BatchEntry *e) { return all.onRound(e); }) != 0) wrong("the walk over all recordings failed");
    if ((int)outs.size() != n) wrong("not one output per recording");
    const int *c = all.route.calls;
    if (c[0] != 1 || c[1] != 1 || c[2] != 1 || c[3] != expand || c[4] != 1 || all.route.mask_sum == 0) wrong("the settings were not made once");
    for (int i = 0; i < n && i < (int)outs.size(); i++) {
      long messages, restarts;
      if (!census(outs[i], &messages, &restarts)) wrong("an output is no well-formed file without raw images");
      if (messages != (long)st[i].published || restarts != (long)st[i].restarts || st[i].rows != 2 * st[i].published) wrong("the records are not as many as the counts");
      if (st[i].raw_images != st[i].dropped + st[i].restarts + st[i].tracked_only + st[i].published || st[i].dropped < 1) wrong("the counts do not add up");
      Node one(1, expand != 0);
      std::vector<std::vector<char>> alone;
      TrackStats s1;
      if (rewriteRecordings(1, paths + i, &alone, &s1, [&](BatchEntry *e) { return one.onRound(e); }) != 0 || alone.size() != 1) {
        wrong("the walk over one recording failed");
        continue;
      }
      if (alone[0] != outs[i]) wrong("a recording alone gives other bytes than among the others");
      s1.tracker_ms = st[i].tracker_ms;
      if (std::memcmp(&s1, &st[i], sizeof s1)) wrong("a recording alone gives other counts than among the others");
      published += (long)st[i].published, images += (long)st[i].raw_images;
    }
    bytes += all.bytes_read;
    if (all.words_drawn % (8 * all.cfg.num_samples) != 0) wrong("words are drawn in whole sets");
  }
  if (published < 1) wrong("nothing was published: the walk compared empty files");
  {  // a round that fails, a file that is missing
    Node node(n, false);
    node.fail_round = 1;
    std::vector<std::vector<char>> outs;
    std::vector<TrackStats> st((size_t)n);
    const int rc = rewriteRecordings(n, paths, &outs, st.data(), [&](BatchEntry *e) { return node.onRound(e); });
    if (rc != -2 || st[0].raw_images != 2 || st[0].dropped != 1) wrong("a failing round");
    std::vector<const char *> with_missing(paths, paths + n);
    const std::string missing = std::string(paths[0]) + ".missing";
    with_missing.push_back(missing.c_str());
    Node more(n + 1, false);
    st.resize((size_t)n + 1);
    if (rewriteRecordings(n + 1, with_missing.data(), &outs, st.data(), [&](BatchEntry *e) { return more.onRound(e); }) != -3 || more.round != 0) wrong("a missing file");
    if (rewriteRecordings(0, paths, &outs, nullptr, [&](BatchEntry *) { return 0; }) != -3) wrong("n = 0");
  }
  std::printf("track_node walk: %d recordings twice, %ld images, %ld published, %ld bytes read, %d wrong\n", n, images, published, bytes, bad);
  return bad ? 1 : 0;
}
