// trace_rewrite.cpp — see trace_rewrite.h.
#include "trace_rewrite.h"

#include <chrono>
#include <cstdint>
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
// One recording being read: every record in front of the next raw image is copied to `out`, the image waits in `buf`
struct Cursor {
  std::FILE *f = nullptr;
  std::vector<char> buf;
  bool pending = false, bad = false;
  ~Cursor() {
    if (f) std::fclose(f);
  }
  void advance(std::vector<char> *out) {
    pending = false;
    for (;;) {
      uint32_t head[2];
      if (std::fread(head, 4, 2, f) != 2) return;
      buf.resize(head[1]);
      if (head[1] && std::fread(buf.data(), 1, head[1], f) != head[1]) {
        bad = true;
        return;
      }
      if (head[0] == 10) {
        pending = true;
        return;
      }
      record(out, head[0], buf.data(), buf.size());
    }
  }
};
}  // namespace

int rewriteRecordings(int n, const char *const *in_paths, std::vector<std::vector<char>> *outs, TrackStats *stats,
                      const std::function<int(BatchEntry *)> &round) {
  if (n < 1) return -3;
  std::vector<TrackStats> st((size_t)n);
  std::memset(st.data(), 0, (size_t)n * sizeof(TrackStats));
  auto finish = [&](int rc) {
    if (stats)
      for (int i = 0; i < n; i++) stats[i] = st[i];
    return rc;
  };
  outs->assign((size_t)n, std::vector<char>());
  std::vector<Cursor> cur((size_t)n);
  for (int i = 0; i < n; i++) {
    {
      Trace check;  // every refusal of the loader is this call's: the pass below trusts the lengths
      if (!check.load(in_paths[i])) return finish(-3);
    }
    cur[i].f = std::fopen(in_paths[i], "rb");
    char file_head[8];
    if (!cur[i].f || std::fread(file_head, 1, 8, cur[i].f) != 8) return finish(-3);
    put(&(*outs)[i], file_head, 8);
    cur[i].advance(&(*outs)[i]);
    if (cur[i].bad) return finish(-3);
  }
  std::vector<BatchEntry> entries((size_t)n);
  for (;;) {
    bool any = false;
    for (int i = 0; i < n; i++) {
      BatchEntry &e = entries[i];
      e.present = cur[i].pending;
      if (!e.present) continue;
      any = true;
      uint32_t dims[4];  // width, height, step, encoding
      std::memcpy(&e.stamp, cur[i].buf.data(), 8), std::memcpy(dims, cur[i].buf.data() + 8, 16);
      e.width = (int)dims[0], e.height = (int)dims[1], e.step = (int)dims[2], e.encoding = (int)dims[3];
      e.pixels = (const unsigned char *)cur[i].buf.data() + 24;
      st[i].raw_images++;
    }
    if (!any) break;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = round(entries.data());
    const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    if (rc < 0) return finish(-2);  // no silent continuation
    for (int i = 0; i < n; i++) {
      BatchEntry &e = entries[i];
      if (!e.present) continue;
      st[i].tracker_ms += ms;  // the round's: the streams share the call
      std::vector<char> *out = &(*outs)[i];
      switch (e.result) {
        case TrackResults::DROPPED:
          st[i].dropped++;
          break;
        case TrackResults::RESTART:  // std_msgs/Bool(true) on the restart topic (feature_tracker_node.cpp:44-46)
          st[i].restarts++;
          record(out, 5, &e.stamp, 8);
          break;
        case TrackResults::PUBLISHED: {
          st[i].published++, st[i].rows += (double)e.msg.size();
          struct {
            double t;
            uint32_t n;
          } __attribute__((packed)) mh = {e.msg.t, (uint32_t)e.msg.size()};
          static_assert(sizeof mh == 12, "packed");
          record(out, 2, &mh, sizeof mh, e.msg.v.data(), e.msg.v.size() * sizeof(float));
          break;
        }
        default:  // tracked only, or the first publication, which the node skips
          st[i].tracked_only++;
      }
      cur[i].advance(out);
      if (cur[i].bad) return finish(-3);
    }
  }
  return finish(0);
}

int writeBytes(const char *path, const std::vector<char> &bytes) {
  std::FILE *f = std::fopen(path, "wb");
  if (!f) return -1;
  const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  return std::fclose(f) == 0 && ok ? 0 : -1;
}

}  // namespace lfvio
