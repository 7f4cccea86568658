// image_gate_walk.cpp — a stand-alone walk over lf-vio_amd/host/image_gate.h for a sanitizer build of the host side (no HIP, no GPU,
// nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/host tests/tools/image_gate_walk.cpp -o image_gate_walk
//   ./image_gate_walk
// Streams at 10 to 60 Hz, gaps, backward, repeated, infinite and NaN stamps through onStamp / afterFrame; checks what must hold
// whatever the stamps are — the stamp behind a restart is dropped, the first publication is skipped exactly once, pub_count never
// goes below 0 — and prints the decisions' counts; exit code 1 when one of them does not hold.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "image_gate.h"

using lfvio::ImageGate;

int main() {
  int bad = 0;
  long counts[5] = {0, 0, 0, 0, 0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int freq : {1, 10, 30})
    for (int hz : {10, 15, 20, 30, 60})
      for (double start : {0.0, -3.0, 1403636579.76, 1e15}) {
        std::vector<double> stamps;
        for (int k = 0; k < 300; k++) stamps.push_back(start + (double)k / hz);
        const double last = stamps.back();
        for (double extra : {last, last + 1.0, std::nextafter(last + 1.0, inf), last + 7.0, last - 0.5, last, inf, -inf, nan, last + 8.0, last + 8.1})
          stamps.push_back(extra);
        ImageGate g;
        g.freq = freq;
        bool after_restart = false;
        int first_publications = 0;
        for (double t : stamps) {
          const ImageGate::Stamp s = g.onStamp(t);
          if (s != ImageGate::TRACK) counts[s]++;
          if (after_restart && s != ImageGate::DROP) std::printf("WRONG: the stamp behind a restart was not dropped (%g)\n", t), bad++;
          after_restart = s == ImageGate::RESTART;
          if (s != ImageGate::TRACK) continue;
          const ImageGate::Frame f = g.afterFrame();
          counts[f]++;
          first_publications += f == ImageGate::FIRST_PUBLICATION;
          if ((f != ImageGate::TRACKED_ONLY) != g.publish) std::printf("WRONG: a message without PUB_THIS_FRAME (%g)\n", t), bad++;
          if (g.pub_count < 0) std::printf("WRONG: pub_count %d\n", g.pub_count), bad++;
        }
        if (first_publications != 1) std::printf("WRONG: %d first publications (freq %d, %d Hz)\n", first_publications, freq, hz), bad++;
      }
  std::printf("dropped %ld, restarts %ld, tracked only %ld, first publications %ld, published %ld; %d wrong\n", counts[0], counts[1], counts[2], counts[3],
              counts[4], bad);
  return bad ? 1 : 0;
}
