// image_gate.h — the bookkeeping of img_callback around readImage (feature_tracker/src/feature_tracker_node.cpp:28-62, :113-178):
// the first image dropped, the discontinuity restart, the FREQ gate that decides PUB_THIS_FRAME, the skipped first publication.
// Plain C++ with no dependencies: host/feature_tracker.cpp uses it, tests/test_image_gate.py compiles it alone and holds every
// decision and every state variable to tests/node_ref.py.
#pragma once
#include <cmath>

namespace lfvio {

struct ImageGate {
  enum Stamp { DROP = 0, RESTART = 1, TRACK = 2 };
  enum Frame { TRACKED_ONLY = 2, FIRST_PUBLICATION = 3, PUBLISHED = 4 };

  int freq = 10;  // FREQ
  // the node's globals (:22-26)
  bool first_image_flag = true;
  double first_image_time = 0;
  double last_image_time = 0;
  int pub_count = 1;
  bool init_pub = false;
  bool publish = false;  // PUB_THIS_FRAME of the last stamp that reached the tracker

  // :30-62.  DROP and RESTART: the image does not reach the tracker.  A restart resets nothing of the tracker (the table, the pyramid,
  // n_id) and not init_pub: the reference does not either.
  Stamp onStamp(double t) {
    if (first_image_flag) {
      first_image_flag = false;
      first_image_time = t, last_image_time = t;
      return DROP;
    }
    if (t - last_image_time > 1.0 || t < last_image_time) {
      first_image_flag = true, last_image_time = 0, pub_count = 1;
      return RESTART;
    }
    last_image_time = t;
    const double r = 1.0 * pub_count / (t - first_image_time);  // (a repeated stamp: inf or NaN, neither publishes)
    publish = std::round(r) <= freq;
    if (publish && std::fabs(r - freq) < 0.01 * freq) first_image_time = t, pub_count = 0;
    return TRACK;
  }

  // :113-178, behind readImage of a stamp that gave TRACK: does the message go out?
  Frame afterFrame() {
    if (!publish) return TRACKED_ONLY;
    pub_count++;
    if (!init_pub) {  // "skip the first image; since no optical speed on frist image"
      init_pub = true;
      return FIRST_PUBLICATION;
    }
    return PUBLISHED;
  }
};

}  // namespace lfvio
