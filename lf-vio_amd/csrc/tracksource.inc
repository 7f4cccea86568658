// tracksource.inc — host side of lfvio_track_source_set (include/lfvio.h, DESIGN.md 3y): the tracker calls of the single route take
// their image through the resident map of remap.inc.  Included by lfvio_hip.hip inside its extern "C" block, behind remap.inc and in
// front of klt.inc, whose klt_pyramid fills level 0 with tracksource_run where the setting is on.
//
// The setting is two numbers; everything else is judged per tracker call by tracksource_call_check (tracksource_plan.h) before
// anything is touched.  What a call uploads and what it tracks differ then: TrackImage says both.

// What a tracker call on a W x H image uploads and how level 0 is filled from it
struct TrackImage {
  bool source = false;       // on: the SOURCE image goes up and level 0 is k_remap_gray's
  ImgfmtPlan im = {};        // source off: the W x H image under the format setting
  TrackSourcePlan src = {};  // source on
  size_t bytes() const { return source ? src.bytes : im.bytes; }
};

// nullptr and *t, or why the call is refused: the format's check beside the image that goes up, and the source's own
static const char *track_image_plan(const lfvio_ctx *c, int W, int H, TrackImage *t) {
  t->source = c->tsource.on;
  if (t->source) {
    if (const char *why = tracksource_call_check(c->tsource, c->remap.r, c->imgfmt.get(), W, H)) return why;
    t->src = tracksource_plan(c->tsource, c->imgfmt.get());
    return nullptr;
  }
  if (const char *why = imgfmt_call_check(c->imgfmt, W, H)) return why;
  t->im = imgfmt_plan(c->imgfmt.get(), W, H);
  return nullptr;
}

// The source image at d_src (device: src.g.sh rows of src.g.step bytes) into the W x H grey bytes at level0, on fs: the integer map
// made this geometry's (remap_index_for), then one launch
static int tracksource_run(lfvio_ctx *c, hipStream_t fs, const TrackSourcePlan &src, int W, int H, const unsigned char *d_src, unsigned char *level0) {
  if (int rc = remap_index_for(c, fs, src.g)) return rc;
  remap_gray_launch(fs, src.code, c->remap.index.get(), d_src, level0, (size_t)W * H);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int lfvio_track_source_set(lfvio_ctx *c, const LfvioTrackSource *src) {
  if (!c) return LFVIO_ERR_ARG;
  if (!src) {
    c->tsource.on = false;
    return LFVIO_OK;
  }
  if (const char *why = remap_side_check(src->src_width, src->src_height)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  c->tsource.on = true, c->tsource.sw = src->src_width, c->tsource.sh = src->src_height;
  return LFVIO_OK;
}
