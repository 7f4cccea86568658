// track_batch_plan_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/trackbatch_plan.h for a CPU sanitizer build of the host side
// of lfvio_track_batch_*: it does on the host's memory what trackbatch.inc does with the plan — checks the entries, takes the
// bounds, lays the staging block out, then fills and reads EVERY byte of every segment of a block of exactly `end` bytes, so that an
// offset or a size that is wrong lands outside the allocation, where AddressSanitizer sees it.  Then the download of
// trackframe_plan.h, as both routes run it behind the copy down: per active slot a down segment of exactly `down_stride` bytes with
// every count at its bound, outputs of exactly `capacity` entries, trackframe_counts_check and trackframe_emit.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc tests/tools/track_batch_plan_walk.cpp -o walk && ./walk
//
// Prints the number of layouts walked and exits 0; anything else is a finding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trackbatch_plan.h"

static int fail(const char *what) {
  std::fprintf(stderr, "track_batch_plan_walk: %s\n", what);
  return 1;
}

int main() {
  const int W = 161, H = 123, S = 100, MC = 40;
  const size_t dev_bytes = sizeof(TfDev);
  std::vector<unsigned char> image((size_t)W * H, 117);
  std::vector<unsigned> words((size_t)S * 8, 0x9e3779b9u);
  LfvioCamera cam = {};
  cam.model = LFVIO_CAM_OCAM, cam.c = 1.0;
  long walked = 0, emitted = 0;
  unsigned seed = 12345;
  auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
  for (int slots = 1; slots <= LFVIO_TRACK_BATCH_MAX_SLOTS; slots += (slots < 8 ? 1 : 7)) {
    for (int round = 0; round < 24; round++) {
      std::vector<LfvioTrackFrameIn> in((size_t)slots);
      std::vector<int> counts((size_t)slots);
      for (int i = 0; i < slots; i++) {
        LfvioTrackFrameIn &e = in[(size_t)i];
        e = LfvioTrackFrameIn{};
        const unsigned r = next() >> 8;
        e.width = W, e.height = H, e.image = (r % 4 == 0 && round) ? nullptr : image.data();  // round 0: every slot active
        e.time = 1.0 + round, e.publish = r % 3 != 0, e.camera = &cam;
        e.win_size = 21, e.max_level = 3, e.max_iterations = 30, e.epsilon = 0.01, e.min_eig_threshold = 1e-4, e.border = 1;
        e.max_count = MC, e.quality_level = 0.01, e.min_distance = 10, e.mask_radius = 10;
        e.num_samples = S, e.sample_words = e.publish ? words.data() : nullptr, e.capacity = LFVIO_TRACK_MAX_POINTS;
        counts[(size_t)i] = round % 6 == 5 ? LFVIO_TRACK_MAX_POINTS : (int)((next() >> 8) % (round % 2 ? 200u : 9u));
      }
      if (round == 23)
        for (auto &e : in) e.image = nullptr;  // all idle
      int capacity = MC;  // the smallest the check accepts: the largest bound of the call is all of the caller's arrays
      for (int n0 : counts) capacity = std::max(capacity, n0);
      for (auto &e : in) e.capacity = capacity;
      if (const char *why = trackbatch_frame_check(slots, slots, in.data(), counts.data())) return fail(why);
      if (!trackbatch_frame_check(slots, slots + 1, in.data(), counts.data())) return fail("count != slots accepted");
      const TbBounds bd = trackbatch_bounds(slots, in.data(), counts.data());
      if (!bd.active) {
        if (bd.first != -1 || bd.n0_max || bd.B_max) return fail("bounds of an all-idle call");
        continue;
      }
      for (int rows = 0; rows < 2; rows++) {
        TbShape shape = {};
        shape.slots = slots, shape.publishing = bd.publishing, shape.active = bd.active;
        shape.n0_max = (size_t)bd.n0_max, shape.B_max = (size_t)bd.B_max, shape.S = (size_t)S, shape.max_count = (size_t)MC, shape.pixels = image.size();
        shape.dev_bytes = dev_bytes, shape.rows = rows != 0;
        const TbStage o = trackbatch_stage(shape);
        unsigned char *block = (unsigned char *)std::malloc(o.end);  // exactly `end` bytes: one past is the sanitizer's
        if (!block) return fail("malloc");
        std::memset(block, 0, o.end);
        const size_t N0 = shape.n0_max, B = shape.B_max;
        size_t sum = 0;
        auto touch = [&](size_t at, size_t bytes, unsigned char tag) {  // nobody wrote here before, then it is ours
          for (size_t k = 0; k < bytes; k++) {
            if (block[at + k]) std::abort();
            block[at + k] = tag;
          }
          sum += bytes;
        };
        TbSlot *desc = (TbSlot *)(block + o.desc);
        touch(o.desc, (size_t)slots * sizeof(TbSlot), 1);
        std::memset(desc, 0, (size_t)slots * sizeof(TbSlot));
        for (int i = 0, ka = 0, kp = 0; i < slots; i++) {
          if (!trackbatch_active(in[(size_t)i])) continue;
          desc[i].active = 1, desc[i].cam = track_cam(cam), desc[i].image_k = ka++;
          const size_t at = trackbatch_image_at(o, shape, desc[i].image_k);
          std::memcpy(block + at, in[(size_t)i].image, shape.pixels);
          if (in[(size_t)i].publish) {
            desc[i].words_k = kp++, desc[i].publish = 1;
            std::memcpy(block + trackbatch_words_at(o, shape, desc[i].words_k), in[(size_t)i].sample_words, (size_t)S * 32);
          }
          if (at + shape.pixels > o.in_end) return fail("an image behind in_end");
        }
        std::memset(block + o.in_end, 0, o.end - o.in_end);
        for (int i = 0; i < slots; i++) {
          const size_t m = trackbatch_mid_at(o, i), d = trackbatch_down_at(o, i);
          const size_t mid[][2] = {{o.c1, N0 * 8}, {o.t1, N0 * 16}, {o.t2, N0 * 16}, {o.bl, N0 * 24}, {o.br, N0 * 24}, {o.A, std::max<size_t>(N0, 9) * 72},
                                   {o.score, (size_t)S * 4}, {o.E, (size_t)S * 72}, {o.raw, B * 4}, {o.matched, B * 4}, {o.next, N0 * 8}, {o.status, N0},
                                   {o.samples, (size_t)S * 32}, {o.mask, N0}, {o.kept, N0 * 4}, {o.corners, (size_t)MC * 8}};
          for (auto &s : mid) touch(m + s[0], s[1], 2);
          const size_t down[][2] = {{o.dev, dev_bytes}, {o.table, B * 16}, {o.un, B * 8}, {o.un3d, B * 12}, {o.vel, B * 12}};
          for (auto &s : down) touch(d + s[0], s[1], 3);
          if (rows) touch(d + o.msg, trackframe_message_bytes(B), 4);
          if (d < o.down || d + o.down_stride > o.end) return fail("a down segment outside the range that comes down");
        }
        if (!sum) return fail("nothing walked");
        for (int i = 0; i < slots; i++) {
          const LfvioTrackFrameIn &e = in[(size_t)i];
          if (!trackbatch_active(e)) continue;
          const bool pub = e.publish != 0, msg_down = rows && pub;
          const int n0 = counts[(size_t)i], np = trackframe_bound(n0, MC, pub);
          char *seg = (char *)std::malloc(o.down_stride);  // exactly one slot's segment
          if (!seg) return fail("malloc");
          std::memset(seg, 0x5a, o.down_stride);
          TfDev v = {};
          v.n1 = v.n2 = n0, v.num_points = np, v.num_new = np, v.reject.status = i % 2, v.detect.num_kept = n0, v.detect.num_corners = MC;
          std::memcpy(seg + o.dev, &v, sizeof v);
          if (rows) std::memcpy(seg + o.msg, &np, sizeof np);
          if (!trackframe_counts_check(v, n0, MC, pub, msg_down ? np : 0)) return fail("counts at their bounds refused");
          TfDev w = v;
          w.num_points = np + 1;
          if (trackframe_counts_check(w, n0, MC, pub, 0)) return fail("num_points beyond its bound accepted");
          const size_t cap = (size_t)capacity;
          std::vector<float> pts(cap * 2), un(cap * 2), un3d(cap * 3), vel(cap * 3), mrows(cap * 9);
          std::vector<int> ids(cap), cnt(cap);
          LfvioTrackFrameOut out = {};
          out.pts = pts.data(), out.ids = ids.data(), out.track_cnt = cnt.data(), out.un_pts = un.data(), out.un_pts_3d = un3d.data(), out.velocity_3d = vel.data();
          LfvioTrackMessage msg = {0, mrows.data()};
          if (!trackframe_out_check(&out, rows ? &msg : nullptr)) return fail("out check");
          trackframe_emit(TfDown{(const TfDev *)(seg + o.dev), seg + o.table, B, seg + o.un, seg + o.un3d, seg + o.vel, msg_down ? seg + o.msg : nullptr}, 3, pub, &out,
                          rows ? &msg : nullptr);
          if (out.num_points != np || msg.num_rows != (msg_down ? np : 0)) return fail("emit's counts");
          std::free(seg);
          emitted++;
        }
        std::free(block);
        walked++;
      }
    }
  }
  // the slot's memory: a layout only grows, and what it grew from still fits
  TbImage lay = trackbatch_image(161, 123, 300000);
  for (int k = 0; k < 6; k++) {
    const TbImage need = trackbatch_image(64 << k, 2048 >> k, (size_t)100000 << k);
    const TbImage grown = trackbatch_image_grown(lay, need);
    if (!trackbatch_image_covers(grown, lay) || !trackbatch_image_covers(grown, need)) return fail("a grown layout that does not cover");
    std::vector<unsigned char> slot(grown.stride());
    std::memset(slot.data() + grown.pyr_at(0), 1, grown.pyr), std::memset(slot.data() + grown.pyr_at(1), 2, grown.pyr);
    std::memset(slot.data() + grown.mask_at(), 3, grown.mask), std::memset(slot.data() + grown.work_at(), 4, grown.work);
    lay = grown;
  }
  if (trackbatch_reserve_check(65) == nullptr || trackbatch_reserve_check(0) != nullptr || trackbatch_slot_check(3, 3) == nullptr ||
      trackbatch_slot_check(-1, 3) != nullptr)
    return fail("a reserve or slot check");
  std::printf("track_batch_plan_walk: %ld layouts walked, %ld down segments emitted\n", walked, emitted);
  return 0;
}
