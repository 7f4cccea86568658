// track_batch_source_walk.cpp — a stand-alone walk over lf-vio_amd/csrc/trackbatch_source_plan.h and the TbMaps part of
// trackbatch_plan.h for a sanitizer build of the host side (no HIP, no GPU, nothing loaded into Python):
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I lf-vio_amd/csrc
//       tests/tools/track_batch_source_walk.cpp -o track_batch_source_walk        (one line)
//   ./track_batch_source_walk
// Three slots with three different maps — equirectangular through a small OCam camera, perspective through a pinhole camera whose M
// sends part of the output outside the source, equirectangular again through the OCam camera at another scale — at 131 x 67 (8777
// pixels: 1 mod 4) and 128 x 64 from a 161 x 123 source in every encoding with a padded odd step.  The maps' block has exactly
// slots * TbMaps::stride() bytes, the source exactly src_height * step and level 0 exactly W * H, so a read or a write outside them is
// the sanitizer's to report: the float maps and the integer map of every slot are written where k_remap_build_b / k_remap_index_b
// write them, then EVERY lane of k_remap_gray_b's launch runs through trackbatch_source_lane; the result against imgfmt_to_gray of the
// host's nearest remap through that slot's own map.  Then every refusal of trackbatch_source_check beside an accepted neighbour, the
// layout's alignment at three sizes and 1, 3 and 64 slots, growth, and the rebuild decision.  Exit code 1 when something is not as
// expected.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "trackbatch_source_plan.h"

static int bad = 0;
static void wrong(const char *what) { std::printf("WRONG: %s\n", what), bad++; }
static const double nan_ = std::numeric_limits<double>::quiet_NaN();

static LfvioCamera blank(int model) {  // everything NaN: a field the header must not read
  LfvioCamera k;
  k.model = model, k.cx = k.cy = k.c = k.d = k.e = k.fx = k.fy = k.k1 = k.k2 = k.p1 = k.p2 = k.xi = nan_;
  for (double &p : k.poly) p = nan_;
  return k;
}
// the PAL camera of an image s times smaller (pixel quantities divided by s)
static void pal_of(double s, LfvioCamera &pal, LfvioProjector &proj) {
  const double poly[5] = {-2.445239e+02, 0.0, 1.748610e-03, -1.757770e-06, 4.475965e-09};
  const double inv[14] = {376.845565, 246.746504, 19.035187, 23.840497, 18.991943, 6.066253, 1.560387, 5.854280, 3.458320, -1.995166, -1.509264,
                          1.089614, 1.340245, 0.255323};
  pal = blank(LFVIO_CAM_OCAM);
  pal.cx = 645.107791 / s, pal.cy = 486.025172 / s, pal.c = 1.0, pal.d = 0.0, pal.e = 0.0;
  double sp = 1.0 / s;
  for (int i = 0; i < 5; i++) pal.poly[i] = poly[i] * sp, sp *= s;
  proj.camera = &pal;
  for (int i = 0; i < LFVIO_OCAM_INV_POLY_SIZE; i++) proj.inv_poly[i] = i < 14 ? inv[i] / s : 0.0;
}

int main() {
  const int SW = 161, SH = 123, SLOTS = 3;
  LfvioCamera pal, pal2, pin = blank(LFVIO_CAM_PINHOLE);
  LfvioProjector proj[SLOTS];
  pal_of(1280.0 / SW, pal, proj[0]);
  pal_of(1.15 * 1280.0 / SW, pal2, proj[2]);
  pin.fx = 461.6 / (752.0 / SW), pin.fy = 460.3 / (752.0 / SW), pin.cx = 363.0 / (752.0 / SW), pin.cy = 248.1 / (752.0 / SW), pin.k1 = pin.k2 = pin.p1 = pin.p2 = 0.0;
  proj[1].camera = &pin;
  for (double &v : proj[1].inv_poly) v = nan_;
  for (const LfvioProjector &p : proj)
    if (proj_check(&p)) wrong("a projector of the walk is refused");
  const double M[9] = {1.0 / pin.fx, 0.0, (-20.0 - pin.cx) / pin.fx, 0.0, 1.0 / pin.fy, (70.0 - pin.cy) / pin.fy, 0.0, 0.0, 1.0};
  const int kinds[SLOTS] = {LFVIO_MAP_EQUIRECT, LFVIO_MAP_PERSPECTIVE, LFVIO_MAP_EQUIRECT};

  const int encodings[] = {LFVIO_IMG_MONO8, LFVIO_IMG_BGR8, LFVIO_IMG_RGB8, LFVIO_IMG_BGRA8, LFVIO_IMG_RGBA8, LFVIO_IMG_MONO16, LFVIO_IMG_MONO16_BE};
  long pixels_done = 0, inside_all = 0, outside_all = 0, lanes_all = 0, rebuilds = 0;
  for (int size = 0; size < 2; size++) {
    const int W = size ? 128 : 131, H = size ? 64 : 67;
    const size_t n = (size_t)W * H;
    const TbMaps lay = trackbatch_maps(W, H);
    if (!trackbatch_maps_aligned(lay, SLOTS) || lay.stride() < 12 * n) wrong("the maps' layout");
    std::vector<char> maps((size_t)SLOTS * lay.stride());  // exactly the three slots' maps
    TbIndexed rec;
    for (int enc : encodings) {
      const int bpp = imgfmt_bpp(enc);
      const LfvioImageFormat fmt = {enc, SW * bpp + 5 + bpp % 2};
      TrackSourceState st;
      st.on = true, st.sw = SW, st.sh = SH;
      const TrackSourcePlan plan = tracksource_plan(st, &fmt);
      // k_remap_build_b's place for every slot (the float maps, and the integer map where the record has a geometry), then
      // k_remap_index_b's where the decision says so
      const RemapGeom at_build = trackbatch_build_geom(rec);
      for (int slot = 0; slot < SLOTS; slot++) {
        char *base = maps.data() + (size_t)slot * lay.stride();
        float *mx = (float *)(base + lay.x_at()), *my = (float *)(base + lay.y_at());
        int *imap = (int *)(base + lay.index_at());
        const ProjCam pc = proj_cam(proj[slot]);
        for (int j = 0; j < H; j++)
          for (int i = 0; i < W; i++) {
            const RemapEntry e = remap_entry(pc, kinds[slot], W, H, M, i, j);
            const size_t p = (size_t)j * W + i;
            mx[p] = e.x, my[p] = e.y;
            if (at_build.bpp) imap[p] = remap_offset(e.x, e.y, at_build);
          }
      }
      const bool need = trackbatch_needs_index(rec, plan.g);  // (bgr8 and rgb8 share a geometry, and so on: then the build's is it)
      if (need != (!rec.indexed || !(rec.geom == plan.g))) wrong("the rebuild decision");
      rebuilds += need;
      for (int slot = 0; need && slot < SLOTS; slot++) {
        char *base = maps.data() + (size_t)slot * lay.stride();
        const float *mx = (const float *)(base + lay.x_at()), *my = (const float *)(base + lay.y_at());
        int *imap = (int *)(base + lay.index_at());
        for (size_t p = 0; p < n; p++) imap[p] = remap_offset(mx[p], my[p], plan.g);
      }
      rec.indexed = true, rec.geom = plan.g;
      if (trackbatch_needs_index(rec, plan.g)) wrong("a steady stream rebuilds");
      std::vector<unsigned char> src(plan.bytes);
      for (size_t k = 0; k < src.size(); k++) src[k] = (unsigned char)(1 + (k * 7 + k / 251) % 255);
      std::vector<std::vector<unsigned char>> all;
      for (int slot = 0; slot < SLOTS; slot++) {
        const int *imap = trackbatch_slot_index(maps.data(), lay, slot);
        std::vector<unsigned char> level0(n), remapped(n * (size_t)bpp), want(n);
        long inside = 0;
        for (size_t p = 0; p < n; p++) {
          const int o = imap[p];
          if (o >= 0 && (size_t)o + (size_t)bpp > src.size()) wrong("an offset behind the source image");
          for (int k = 0; k < bpp; k++) remapped[p * (size_t)bpp + k] = o < 0 ? 0 : src[(size_t)o + k];
          inside += o >= 0;
        }
        if (inside == 0 || inside == (long)n) wrong("a map without inside or without outside entries");
        imgfmt_to_gray(enc, W, H, (size_t)W * bpp, remapped.data(), want.data());
        const size_t lanes = tracksource_lanes(n);
        for (size_t lane = 0; lane < lanes; lane++) trackbatch_source_lane(enc, maps.data(), lay, slot, src.data(), level0.data(), n, lane);
        if (level0 != want) wrong("level 0 is not the grey image of the remapped one");
        all.push_back(level0);
        pixels_done += (long)n, inside_all += inside, outside_all += (long)n - inside, lanes_all += (long)lanes;
      }
      if (all[0] == all[1] || all[1] == all[2] || all[0] == all[2]) wrong("two slots gave the same image: three maps, not one");
    }
  }

  // the per-call check
  {
    static const unsigned char pixel = 0;
    TrackSourceState off, on;
    on.on = true, on.sw = SW, on.sh = SH;
    LfvioTrackFrameIn in[3];
    std::memset(in, 0, sizeof in);
    for (LfvioTrackFrameIn &f : in) f.image = &pixel, f.width = 131, f.height = 67;
    TbMapInfo maps[3];
    for (TbMapInfo &m : maps) m.valid = true, m.width = 131, m.height = 67;
    const LfvioImageFormat bgr = {LFVIO_IMG_BGR8, 0}, bad_code = {1, 0}, short_step = {LFVIO_IMG_BGR8, 482}, exact = {LFVIO_IMG_BGR8, 483};
    if (trackbatch_source_check(on, &bgr, 3, in, maps) || trackbatch_source_check(on, nullptr, 3, in, maps) || trackbatch_source_check(on, &exact, 3, in, maps))
      wrong("a valid call is refused");
    if (!trackbatch_source_check(on, &short_step, 3, in, maps) || !trackbatch_source_check(on, &bad_code, 3, in, maps)) wrong("a format is not judged beside the source");
    maps[1].valid = false;
    if (!trackbatch_source_check(on, &bgr, 3, in, maps)) wrong("an active slot without a map is accepted");
    if (trackbatch_source_check(off, &bad_code, 3, in, maps)) wrong("the setting off refuses");
    in[1].image = nullptr;
    if (trackbatch_source_check(on, &bgr, 3, in, maps)) wrong("an idle slot needs a map");
    maps[2].width = 128, maps[2].height = 64;
    if (!trackbatch_source_check(on, &bgr, 3, in, maps)) wrong("a map of another size is accepted");
    in[2].image = nullptr;
    if (trackbatch_source_check(on, &bgr, 3, in, maps)) wrong("an idle slot's map of another size refuses");
    for (int side : {15, 8193, 0, -1}) {
      TrackSourceState t = on;
      t.sw = side;
      if (!trackbatch_source_check(t, &bgr, 3, in, maps) || !trackbatch_source_set_check(side, SH)) wrong("a source width outside [16, 8192] is accepted");
      t.sw = SW, t.sh = side;
      if (!trackbatch_source_check(t, nullptr, 3, in, maps) || !trackbatch_source_set_check(SW, side)) wrong("a source height outside [16, 8192] is accepted");
    }
    if (trackbatch_source_set_check(16, 8192)) wrong("16 or 8192 is refused");
  }

  // the layout at three sizes and 1, 3 and 64 slots; growth; the rebuild decision beside remap_needs_index
  long layouts = 0;
  for (int slots : {1, 3, 64})
    for (int size = 0; size < 3; size++) {
      const int W = size == 0 ? 131 : size == 1 ? 128 : 17, H = size == 0 ? 67 : size == 1 ? 64 : 16;
      const TbMaps m = trackbatch_maps(W, H);
      if (!trackbatch_maps_aligned(m, slots) || m.plane() < (size_t)W * H * 4 || m.y_at() != m.plane() || m.index_at() != 2 * m.plane() || m.stride() != 3 * m.plane())
        wrong("the maps' layout");
      if (!trackbatch_level0_aligned(trackbatch_image(W, H, gft_work(W, H).bytes), slots)) wrong("level 0 is not 4-aligned");
      const TbMaps g = trackbatch_maps_grown(m, trackbatch_maps(131, 67));
      if (!trackbatch_maps_covers(g, m) || !trackbatch_maps_covers(g, trackbatch_maps(131, 67)) || g.px != 131 * 67) wrong("growth");
      layouts++;
    }
  {
    const RemapGeom geoms[] = {{1280, 960, 3840, 3}, {1281, 960, 3843, 3}, {1280, 961, 3840, 3}, {1280, 960, 3844, 3}, {1280, 960, 5120, 4}, {1280, 960, 1280, 1}};
    for (const RemapGeom &have : geoms)
      for (const RemapGeom &now : geoms)
        for (bool indexed : {false, true}) {
          TbIndexed r;
          r.indexed = indexed, r.geom = have;
          RemapResident one;
          one.valid = true, one.indexed = indexed, one.geom = have;
          if (trackbatch_needs_index(r, now) != remap_needs_index(one, now)) wrong("the rebuild decision is not remap_needs_index");
          const RemapGeom b = trackbatch_build_geom(r);
          if (indexed ? !(b == have) : b.bpp != 0) wrong("the geometry a build writes for");
        }
  }
  if (rebuilds != 8) wrong("the walk rebuilt the integer maps another number of times than 4 geometries x 2 sizes");
  std::printf("track_batch_source walk: %ld pixels through %ld lanes (%ld inside, %ld outside), %ld rebuilds, %ld layouts, %d wrong\n", pixels_done, lanes_all,
              inside_all, outside_all, rebuilds, layouts, bad);
  return bad ? 1 : 0;
}
