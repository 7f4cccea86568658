// trace_rewrite.h — recordings with raw images (record type 10 of replay.h) rewritten: every image replaced by what the node published
// at that place — a feature message (type 2), a restart (type 5, with the stamp) or nothing — and every other record copied byte for
// byte.  ONE walk for one recording (image_replay.h) and for n in lockstep (batch_tracker.h); what tracks the images is the caller's
// round callback, so nothing here names a device symbol.  tests/test_trace_rewrite.py runs it with a stub round.
#pragma once
#include <functional>
#include <vector>

#include "replay.h"
#include "track_node.h"

namespace lfvio {

struct TrackStats {
  double raw_images, dropped, restarts, tracked_only /* the skipped first publication included */, published, rows, tracker_ms;
};

// One stream's image of a round (present = false: the stream has none), and what became of it
struct BatchEntry {
  bool present = false;
  double stamp = 0;
  int width = 0, height = 0, step = 0, encoding = LFVIO_IMG_MONO8;
  const unsigned char *pixels = nullptr;
  int result = TrackResults::DROPPED;  // a TrackResults::Result; PUBLISHED: msg is the feature message, stamped `stamp`
  TraceImage msg;
};

// n recordings walked in lockstep: round r takes the r-th raw image of every recording that still has one, as entries[n] to `round`,
// which sets every present entry's result (and msg) and returns 0, or a negative value that ends the walk.  outs[i]: the bytes of the
// LFVT file that recording i becomes; stats[n] (or null), tracker_ms: of the rounds the recording took part in, raw_images: counted
// before the round.  0; -3: n < 1, or a recording is unreadable or refused by Trace::load; -2: `round` returned a negative value.  On
// anything but 0 the outs are not to be used.
int rewriteRecordings(int n, const char *const *in_paths, std::vector<std::vector<char>> *outs, TrackStats *stats,
                      const std::function<int(BatchEntry *)> &round);

// 0, or -1: cannot write
int writeBytes(const char *path, const std::vector<char> &bytes);

}  // namespace lfvio
