// trackbatch.inc — host side of the lfvio_track_batch_* calls (include/lfvio.h): lfvio_track_frame_message for every slot of the
// batch in the launches of ONE frame.  The kernels are those of kernels_trackbatch.h, the single route's device functions with the
// slot in blockIdx.z; the checks, the bounds and every offset come from trackbatch_plan.h.  Included by lfvio_hip.hip inside its
// extern "C" block, behind trackframe.inc.
//
// One call: check every entry, size grids and segments for the batch's bounds (n0_max, B_max), fill the descriptors, ONE copy up of
// [descriptors | words | images], the launches of trackframe.inc once each with grid.z = slots, ONE copy down of every slot's down
// segment.  Only then, with every count checked against its bound, are the outputs written and the double buffers of the active
// slots swapped: a call that is refused or fails leaves every output and every slot as it was.
//
// On the expanded image (lfvio_track_batch_map, lfvio_track_batch_source; DESIGN.md 3z; the checks, the rebuild decision and the
// maps' layout from trackbatch_source_plan.h / trackbatch_plan.h): every slot has a resident remap in a block of the batch's own, the
// images that go up are the SOURCE images, and level 0 of every slot is one k_remap_gray_b launch through the slot's integer map —
// behind at most one k_remap_index_b launch where the source geometry is not the one the integer maps were written for.

static int tb_copy(lfvio_ctx *c, hipStream_t fs, const char *src, size_t sstride, char *dst, size_t dstride, size_t bytes, int n) {
  if (!bytes || n < 1) return LFVIO_OK;
  hipLaunchKernelGGL(k_tb_copy, dim3((unsigned)((bytes + TB_COPY_BYTES - 1) / TB_COPY_BYTES), 1, n), dim3(TB_COPY_THREADS), 0, fs, (const unsigned char *)src,
                     sstride, (unsigned char *)dst, dstride, bytes);
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

// The slots' image blocks with at least the capacities of `need`.  A block that has to grow is allocated beside the old one, the
// pyramids and the masks move over, then it replaces the old one: a failure leaves the batch as it was.
static int tb_image_reserve(lfvio_ctx *c, hipStream_t fs, const TbImage &need) {
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  if (b.image && trackbatch_image_covers(b.lay, need)) return LFVIO_OK;
  const int n = (int)b.slot.size();
  const TbImage lay = b.image ? trackbatch_image_grown(b.lay, need) : need;
  DevBuf<char> fresh;
  if (!fresh.reserve((size_t)n * lay.stride())) return out_of_memory(c, "out of memory (track batch images)");
  if (b.image) {
    for (int which = 0; which < 2; which++)
      if (int rc = tb_copy(c, fs, b.image + b.lay.pyr_at(which), b.lay.stride(), fresh + lay.pyr_at(which), lay.stride(), b.lay.pyr, n)) return rc;
    if (int rc = tb_copy(c, fs, b.image + b.lay.mask_at(), b.lay.stride(), fresh + lay.mask_at(), lay.stride(), b.lay.mask, n)) return rc;
    HIPCHK(c, hipStreamSynchronize(fs));
  }
  b.image = std::move(fresh), b.lay = lay;
  return LFVIO_OK;
}

// The slots' maps with at least the capacity of `need`, as tb_image_reserve: a block that has to grow is allocated beside the old
// one, every slot's three planes move over, then it replaces the old one — a failure leaves the previous maps usable.
static int tb_maps_reserve(lfvio_ctx *c, hipStream_t fs, const TbMaps &need) {
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  if (b.maps && trackbatch_maps_covers(b.mlay, need)) return LFVIO_OK;
  const int n = (int)b.slot.size();
  const TbMaps lay = b.maps ? trackbatch_maps_grown(b.mlay, need) : need;
  DevBuf<char> fresh;
  if (!fresh.reserve((size_t)n * lay.stride())) return out_of_memory(c, "out of memory (track batch maps)");
  if (b.maps) {
    const size_t from[3] = {b.mlay.x_at(), b.mlay.y_at(), b.mlay.index_at()}, to[3] = {lay.x_at(), lay.y_at(), lay.index_at()};
    for (int k = 0; k < 3; k++)
      if (int rc = tb_copy(c, fs, b.maps + from[k], b.mlay.stride(), fresh + to[k], lay.stride(), b.mlay.plane(), n)) return rc;
    HIPCHK(c, hipStreamSynchronize(fs));
  }
  b.maps = std::move(fresh), b.mlay = lay;
  return LFVIO_OK;
}
// where the slots' maps lie, for the kernels
static void tb_maps_mem(const lfvio_ctx::TrackBatchState &b, TbMem &m) {
  m.maps = b.maps.get(), m.maps_stride = b.mlay.stride(), m.maps_y_at = b.mlay.y_at(), m.maps_index_at = b.mlay.index_at();
}

int lfvio_track_batch_map(lfvio_ctx *c, int slot, const LfvioRemapIn *in) {
  if (!c) return LFVIO_ERR_ARG;
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  const int n = (int)b.slot.size();
  if (const char *why = trackbatch_slot_check(slot, n)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int first = slot < 0 ? 0 : slot, last = slot < 0 ? n : slot + 1;
  if (!in) {
    for (int i = first; i < last; i++) b.map[i] = TbMapInfo();
    return LFVIO_OK;
  }
  if (const char *why = remap_build_check(in, nullptr, nullptr)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const TbMaps need = trackbatch_maps(in->width, in->height);
  if (!trackbatch_maps_aligned(b.maps ? trackbatch_maps_grown(b.mlay, need) : need, n)) {  // (true by construction; before anything is touched)
    c->err = "lfvio_track_batch_map: a slot's maps are not 256-aligned";
    return LFVIO_ERR_DEVICE;
  }
  FeatStage st(c);
  if (int rc = tb_maps_reserve(c, st.fs, need)) return rc;
  RemapBuildArgs a = {};
  a.cam = proj_cam(*in->proj, &b.map_kb);
  a.kind = in->kind, a.width = in->width, a.height = in->height;
  for (int k = 0; k < 9; k++) a.M[k] = in->kind == LFVIO_MAP_PERSPECTIVE ? in->M[k] : 0.0;
  a.g = trackbatch_build_geom(b.indexed);  // of the batch's frames (bpp 0: there was none yet, and the first one writes every integer map)
  for (int i = first; i < last; i++) b.map[i].valid = false;  // until the new maps are enqueued: a failure below leaves no map, not a stale one
  TbMem m = {};
  tb_maps_mem(b, m);
  const RemapGrid g = remap_build_grid(in->width, in->height);
  hipLaunchKernelGGL(k_remap_build_b, dim3(g.x, g.y, (unsigned)(last - first)), dim3(REMAP_THREADS), 0, st.fs, a, m, first);
  HIPCHK(c, hipGetLastError());
  for (int i = first; i < last; i++) b.map[i].valid = true, b.map[i].width = in->width, b.map[i].height = in->height;
  return LFVIO_OK;
}

int lfvio_track_batch_source(lfvio_ctx *c, const LfvioTrackSource *src) {
  if (!c) return LFVIO_ERR_ARG;
  if (!src) {
    c->tbatch.source.on = false;
    return LFVIO_OK;
  }
  if (const char *why = trackbatch_source_set_check(src->src_width, src->src_height)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  c->tbatch.source.on = true, c->tbatch.source.sw = src->src_width, c->tbatch.source.sh = src->src_height;
  return LFVIO_OK;
}

// lfvio_klt_level for a slot: level `level` of the slot's resident pyramid
int lfvio_track_batch_level(lfvio_ctx *c, int slot, int level, int *width, int *height, unsigned char *pixels) {
  if (!c || !width || !height) return LFVIO_ERR_ARG;
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  const int n = (int)b.slot.size();
  const bool in_range = slot >= 0 && slot < n;
  if (const char *why = trackbatch_level_check(slot, n, in_range && b.slot[slot].valid && b.image, level, in_range ? b.slot[slot].built : 0)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const TrackStream &k = b.slot[slot];
  const KltPlan full = klt_plan(k.w, k.h, 0, LFVIO_KLT_MAX_LEVEL);
  if (pixels) {
    FeatStage st(c);
    HIPCHK(c, hipMemcpyAsync(pixels, b.image + (size_t)slot * b.lay.stride() + b.lay.pyr_at(k.pcur) + full.off[level], (size_t)full.w[level] * full.h[level],
                             hipMemcpyDeviceToHost, st.fs));
    HIPCHK(c, hipStreamSynchronize(st.fs));
  }
  *width = full.w[level], *height = full.h[level];
  return LFVIO_OK;
}

int lfvio_track_batch_reserve(lfvio_ctx *c, int slots) {
  if (!c) return LFVIO_ERR_ARG;
  if (const char *why = trackbatch_reserve_check(slots)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  FeatStage st(c);
  DevBuf<char> fresh;
  if (slots && !fresh.reserve((size_t)slots * TB_FIXED_BYTES)) return out_of_memory(c, "out of memory (track batch slots)");
  HIPCHK(c, hipStreamSynchronize(st.fs));
  b.fixed = std::move(fresh);
  (void)b.image.reset(), (void)b.clahe.reset();
  b.lay = TbImage{0, 0, 0}, b.clahe_dirty = false;
  b.slot.assign((size_t)slots, TrackStream());
  b.kb.assign((size_t)slots, KbCache());
  // no slot has a map, as a fresh context has none (the source setting, which is the batch's, stays)
  (void)b.maps.reset();
  b.mlay = TbMaps{0}, b.indexed = TbIndexed();
  b.map.assign((size_t)slots, TbMapInfo());
  return LFVIO_OK;
}

int lfvio_track_batch_reset(lfvio_ctx *c, int slot) {
  if (!c) return LFVIO_ERR_ARG;
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  if (const char *why = trackbatch_slot_check(slot, (int)b.slot.size())) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  for (int i = 0; i < (int)b.slot.size(); i++)
    if (slot < 0 || i == slot) b.slot[i].reset_frame();
  return LFVIO_OK;
}

int lfvio_track_batch_clahe(lfvio_ctx *c, const LfvioClaheIn *cfg) {
  if (!c) return LFVIO_ERR_ARG;
  if (!cfg) {
    c->tbatch.clahe_on = false;
    return LFVIO_OK;
  }
  if (const char *why = clahe_check(cfg)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  c->tbatch.cfg = *cfg, c->tbatch.clahe_on = true;
  return LFVIO_OK;
}

int lfvio_track_batch_format(lfvio_ctx *c, const LfvioImageFormat *fmt) {
  if (!c) return LFVIO_ERR_ARG;
  return imgfmt_set(c, c->tbatch.imgfmt, fmt);
}

int lfvio_track_batch_set_mask(lfvio_ctx *c, int slot, int width, int height, const unsigned char *pixels) {
  if (!c) return LFVIO_ERR_ARG;
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  const int n = (int)b.slot.size();
  if (const char *why = trackbatch_slot_check(slot, n)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const int first = slot < 0 ? 0 : slot, last = slot < 0 ? n : slot + 1;
  if (!pixels) {
    for (int i = first; i < last; i++) b.slot[i].mask_cleared();
    return LFVIO_OK;
  }
  for (int i = first; i < last; i++)
    if (const char *why = gft_mask_check(width, height, b.slot[i].resident_w(), b.slot[i].h)) {
      c->err = why;
      return LFVIO_ERR_ARG;
    }
  const size_t px = (size_t)width * height;
  FeatStage st(c);
  const size_t oM = st.take(px);
  if (int rc = st.reserve()) return rc;
  if (int rc = tb_image_reserve(c, st.fs, trackbatch_image(width, height, 0))) return rc;
  std::memcpy(st.h + oM, pixels, px);
  if (int rc = st.up(st.end)) return rc;
  if (int rc = tb_copy(c, st.fs, st.d + oM, 0, b.image + (size_t)first * b.lay.stride() + b.lay.mask_at(), b.lay.stride(), px, last - first)) return rc;
  HIPCHK(c, hipStreamSynchronize(st.fs));
  for (int i = first; i < last; i++) b.slot[i].mask_is(width, height);
  return LFVIO_OK;
}

int lfvio_track_batch_frame(lfvio_ctx *c, int count, const LfvioTrackFrameIn *in, LfvioTrackFrameOut *out, LfvioTrackMessage *msg) {
  if (!c) return LFVIO_ERR_ARG;
  if (!in || !out) {
    c->err = "lfvio_track_batch_frame: null in or out";
    return LFVIO_ERR_ARG;
  }
  lfvio_ctx::TrackBatchState &b = c->tbatch;
  const int n = (int)b.slot.size();
  int counts[LFVIO_TRACK_BATCH_MAX_SLOTS];
  for (int i = 0; i < n; i++) counts[i] = b.slot[i].count;
  if (const char *why = trackbatch_frame_check(n, count, in, counts)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  for (int i = 0; i < n; i++) {
    if (!trackbatch_active(in[i])) continue;
    if (!trackframe_out_check(&out[i], msg ? &msg[i] : nullptr) || (in[i].publish && !b.slot[i].mask_fits(in[i].width, in[i].height))) {
      c->err = "lfvio_track_batch_frame: a null array in out or msg, or a base mask that is not the image's size";
      return LFVIO_ERR_ARG;
    }
  }
  const TbBounds bd = trackbatch_bounds(n, in, counts);
  if (!bd.active) {  // nothing to do, and nothing on the device
    for (int i = 0; i < n; i++) {
      trackframe_zero(&out[i]);
      if (msg) msg[i].num_rows = 0;
    }
    return LFVIO_OK;
  }
  const LfvioTrackFrameIn &f = in[bd.first];  // the shared fields
  const int W = f.width, H = f.height, S = f.num_samples, MC = f.max_count;
  // what goes up: the W x H images under the format setting, or under lfvio_track_batch_source the SOURCE images, whose check is
  // the slots' maps and the format beside the source's size
  const bool source = b.source.on;
  if (const char *why = source ? trackbatch_source_check(b.source, b.imgfmt.get(), n, in, b.map.data()) : imgfmt_call_check(b.imgfmt, W, H)) {
    c->err = why;
    return LFVIO_ERR_ARG;
  }
  const ImgfmtPlan im = imgfmt_plan(b.imgfmt.get(), W, H);  // (source on: not looked at)
  const TrackSourcePlan sp = source ? tracksource_plan(b.source, b.imgfmt.get()) : TrackSourcePlan{};
  const LfvioKltIn kin = trackframe_klt(&f);
  const LfvioGftIn gin = trackframe_gft(&f);
  const KltPlan full = klt_plan(W, H, 0, LFVIO_KLT_MAX_LEVEL);
  const int LU = klt_plan(W, H, f.win_size, f.max_level).levels_used;
  const GftWork gw = gft_work(W, H);
  const GftOffsets &wk = gw;  // what the kernels take
  const size_t nI = source ? sp.bytes : im.bytes;  // of one staged image; level 0 has W * H
  const bool rows = msg != nullptr, any_pub = bd.publishing > 0;
  TbShape shape = {};
  shape.slots = n, shape.publishing = bd.publishing, shape.active = bd.active;
  shape.n0_max = (size_t)bd.n0_max, shape.B_max = (size_t)bd.B_max, shape.S = (size_t)S, shape.max_count = (size_t)MC, shape.pixels = nI;
  shape.dev_bytes = sizeof(TfDev), shape.rows = rows;
  const TbStage o = trackbatch_stage(shape);
  // what k_remap_gray_b's dword store and int4 load rest on (TbMaps, trackbatch_plan.h), on the layout this call will run on: true by
  // construction, and judged like every other refusal before anything is touched
  const TbImage need = trackbatch_image(W, H, gw.bytes);
  if (source && !(trackbatch_level0_aligned(b.image ? trackbatch_image_grown(b.lay, need) : need, n) && trackbatch_maps_aligned(b.mlay, n))) {
    c->err = "lfvio_track_batch_frame: level 0 or a slot's integer map is not aligned";
    return LFVIO_ERR_DEVICE;
  }
  FeatStage st(c);
  st.end = o.end;
  if (int rc = st.reserve()) return rc;
  if (int rc = tb_image_reserve(c, st.fs, need)) return rc;
  if (b.clahe_on) {
    if (!b.clahe) {
      if (!b.clahe.reserve((size_t)n * (CLAHE_TABLE_BYTES + CLAHE_LUT_BYTES))) return out_of_memory(c, "out of memory (CLAHE)");
      b.clahe_dirty = true;
    }
    if (b.clahe_dirty) {  // fresh memory, or a call that failed between the histograms and the LUTs
      HIPCHK(c, hipMemsetAsync(b.clahe, 0, (size_t)n * (CLAHE_TABLE_BYTES + CLAHE_LUT_BYTES), st.fs));
      b.clahe_dirty = false;
    }
  }
  char *d = st.d, *h = st.h;
  const TbImage &lay = b.lay;
  TbMem m = {};
  m.stage = d, m.fixed = b.fixed, m.image = b.image, m.clahe = b.clahe_on ? b.clahe.get() : nullptr;
  m.image_stride = lay.stride(), m.pyr = lay.pyr, m.mask_at = lay.mask_at(), m.work_at = lay.work_at(), m.clahe_stride = CLAHE_TABLE_BYTES + CLAHE_LUT_BYTES;
  m.words_at = o.words, m.words_stride = trackbatch_words_at(o, shape, 1) - o.words, m.images_at = o.images, m.images_stride = trackbatch_image_at(o, shape, 1) - o.images;
  tb_maps_mem(b, m);
  TbSlot *desc = (TbSlot *)(h + o.desc);
  std::memset(desc, 0, (size_t)n * sizeof(TbSlot));
  bool build_resident = false;
  size_t map_px_max = 0;  // the largest resident map, idle slots' too
  for (int i = 0, ka = 0, kp = 0; i < n; i++) {
    if (source && b.map[i].valid) {
      desc[i].map_px = b.map[i].width * b.map[i].height;
      map_px_max = std::max(map_px_max, (size_t)desc[i].map_px);
    }
    if (!trackbatch_active(in[i])) continue;
    TbSlot &t = desc[i];
    t.active = 1, t.publish = in[i].publish != 0;
    trackbatch_describe(t, b.slot[i], W, H, LU, in[i].time);
    t.cam = track_cam(*in[i].camera, &b.kb[i]);
    t.image_k = ka++;
    std::memcpy(h + trackbatch_image_at(o, shape, t.image_k), in[i].image, nI);
    if (t.publish) {
      t.words_k = kp++;
      std::memcpy(h + trackbatch_words_at(o, shape, t.words_k), in[i].sample_words, (size_t)S * 32);
    }
    build_resident = build_resident || b.slot[i].levels_missing(W, H, LU) > 0;
  }
  if (int rc = st.up(o.in_end)) return rc;

  const TbSlot *slots = (const TbSlot *)(d + o.desc);
  const unsigned Z = (unsigned)n;
  hipStream_t fs = st.fs;
  // level 0 of every fresh pyramid: the image (converted to grey under a format, or gathered from the source image through the
  // slot's map), or the equalized image
  const int conv = (source || im.convert) ? 1 : 0;  // level 0 is written by a kernel of its own; CLAHE, if on, reads it there
  if (source) {
    if (trackbatch_needs_index(b.indexed, sp.g)) {  // the integer maps of every mapped slot made this geometry's, in one launch
      b.indexed.indexed = false;
      hipLaunchKernelGGL(k_remap_index_b, dim3((unsigned)((map_px_max + REMAP_THREADS - 1) / REMAP_THREADS), 1, Z), dim3(REMAP_THREADS), 0, fs, slots, m, sp.g);
      HIPCHK(c, hipGetLastError());
      b.indexed.geom = sp.g, b.indexed.indexed = true;
    }
    remap_gray_b_launch(fs, Z, slots, m, o, sp.code, (size_t)W * H);
    HIPCHK(c, hipGetLastError());
  } else if (conv) {
    hipLaunchKernelGGL(k_img_gray_b, dim3((W + IMG_COLS - 1) / IMG_COLS, (H + IMG_ROWS - 1) / IMG_ROWS, Z), dim3(IMG_THREADS), 0, fs, slots, m, o, im.code, im.step, W, H);
    HIPCHK(c, hipGetLastError());
  }
  if (b.clahe_on) {
    const ClahePlan p = clahe_plan(W, H, b.cfg);
    const int tiles = b.cfg.tiles_x * b.cfg.tiles_y, bands = (p.th + CLAHE_BAND_ROWS - 1) / CLAHE_BAND_ROWS;
    b.clahe_dirty = true;
    hipLaunchKernelGGL(k_clahe_hist_b, dim3(tiles, bands, Z), dim3(CLAHE_THREADS), 0, fs, slots, m, o, conv, W, H, b.cfg.tiles_x, p.tw, p.th);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_clahe_lut_b, dim3(tiles, 1, Z), dim3(CLAHE_THREADS), 0, fs, slots, m, o, p.clip, p.lut_scale, CLAHE_TABLE_BYTES);
    HIPCHK(c, hipGetLastError());
    b.clahe_dirty = false;
    const dim3 grid((W + CLAHE_MAP_COLS - 1) / CLAHE_MAP_COLS, (b.cfg.tiles_y + 1) * bands, Z);
    if (W % 4 == 0)
      hipLaunchKernelGGL(k_clahe_map_b<true>, grid, dim3(CLAHE_THREADS), 0, fs, slots, m, o, conv, W, H, b.cfg.tiles_x, b.cfg.tiles_y, p.th, bands, p.inv_tw, p.inv_th,
                         CLAHE_TABLE_BYTES);
    else
      hipLaunchKernelGGL(k_clahe_map_b<false>, grid, dim3(CLAHE_THREADS), 0, fs, slots, m, o, conv, W, H, b.cfg.tiles_x, b.cfg.tiles_y, p.th, bands, p.inv_tw, p.inv_th,
                         CLAHE_TABLE_BYTES);
    HIPCHK(c, hipGetLastError());
  } else if (!conv) {
    hipLaunchKernelGGL(k_tb_image, dim3((unsigned)((nI + TB_COPY_BYTES - 1) / TB_COPY_BYTES), 1, Z), dim3(TB_COPY_THREADS), 0, fs, slots, m, o, nI);
    HIPCHK(c, hipGetLastError());
  }
  // 1: the pyramids (the resident ones too, where an earlier call asked for fewer levels), the flow
  for (int resident = 0; resident < (build_resident ? 2 : 1); resident++)
    for (int k = 1; k <= LU; k++) {
      hipLaunchKernelGGL(k_klt_down_b, dim3((full.w[k] + 63) / 64, (full.h[k] + 3) / 4, Z), dim3(256), 0, fs, slots, m, o, resident, k, full.off[k - 1], full.w[k - 1],
                         full.h[k - 1], full.off[k], full.w[k], full.h[k]);
      HIPCHK(c, hipGetLastError());
    }
  if (bd.n0_max) {
    hipLaunchKernelGGL(k_klt_track_b, dim3(bd.n0_max, 1, Z), dim3(KLT_THREADS), 0, fs, slots, m, o, klt_args(&kin, full, LU));
    HIPCHK(c, hipGetLastError());
  }
  // 2: reduceVector, track_cnt++, the sample sets
  hipLaunchKernelGGL(k_tf_flow_b, dim3(1, 1, Z), dim3(TF_THREADS), 0, fs, slots, m, o, bd.n0_max, S);
  HIPCHK(c, hipGetLastError());
  if (any_pub) {
    // 3: rejectWithF, reduceVector by its mask
    if (bd.n0_max >= TRACK_MIN_MATCHES) {
      hipLaunchKernelGGL(k_trk_lift_b, dim3((2 * bd.n0_max + TRK_THREADS - 1) / TRK_THREADS, 1, Z), dim3(TRK_THREADS), 0, fs, slots, m, o);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_tv_hyp_b, dim3(S, 1, Z), dim3(TV_HYP_THREADS), 0, fs, slots, m, o);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_trk_fit_b, dim3(1, 1, Z), dim3(TV_FIT_THREADS), 0, fs, slots, m, o, S);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_tf_reject_b, dim3(1, 1, Z), dim3(TF_THREADS), 0, fs, slots, m, o, bd.n0_max);
    HIPCHK(c, hipGetLastError());
    // 4: setMask and goodFeaturesToTrack on the new images; the sort network of the arrays' capacity (gft_plan.h)
    hipLaunchKernelGGL(k_gft_thin_b, dim3(1, 1, Z), dim3(GFT_THREADS), 0, fs, slots, m, o, wk, bd.n0_max, W, H, gin.mask_radius);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_gft_response_b, dim3((W + GFT_TX - 1) / GFT_TX, (H + GFT_TY - 1) / GFT_TY, Z), dim3(GFT_THREADS), 0, fs, slots, m, o, wk, W, H, gin.mask_radius, MC);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_gft_cand_b, dim3((W + GFT_THREADS - 1) / GFT_THREADS, (H + GFT_CAND_ROWS - 1) / GFT_CAND_ROWS, Z), dim3(GFT_THREADS), 0, fs, slots, m, o, wk, W, H,
                       gin.quality_level, MC);
    HIPCHK(c, hipGetLastError());
    const GftSortGrid sg = gft_sort_grid(gw.capacity);
    gft_sort_stages(
        gw.capacity, [&](unsigned kk) { hipLaunchKernelGGL(k_gft_sort_local_b, dim3(sg.chunks, 1, Z), dim3(GFT_SORT_THREADS), 0, fs, slots, m, o, wk, kk); },
        [&](unsigned kk, unsigned j) { hipLaunchKernelGGL(k_gft_sort_global_b, dim3(sg.halves, 1, Z), dim3(GFT_THREADS), 0, fs, slots, m, o, wk, kk, j); });
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_gft_pick_b, dim3(1, 1, Z), dim3(GFT_THREADS), 0, fs, slots, m, o, wk, W, gin.min_distance, MC);
    HIPCHK(c, hipGetLastError());
  }
  // 4 and 6: the next tables, numbered; 5: undistortedPoints; the messages
  hipLaunchKernelGGL(k_tf_finish_b, dim3(1, 1, Z), dim3(TF_THREADS), 0, fs, slots, m, o, bd.n0_max, bd.B_max);
  HIPCHK(c, hipGetLastError());
  if (bd.B_max) {
    hipLaunchKernelGGL(k_trk_undist_b, dim3((bd.B_max + TRK_THREADS - 1) / TRK_THREADS, 1, Z), dim3(TRK_THREADS), 0, fs, slots, m, o);
    HIPCHK(c, hipGetLastError());
  }
  if (rows && any_pub) {
    hipLaunchKernelGGL(k_tf_message_b, dim3(1, 1, Z), dim3(TF_THREADS), 0, fs, slots, m, o, bd.B_max);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.down(o.down, o.end)) return rc;

  // every count of every active slot against its own bound, before anything is written
  auto rows_at = [&](int i) { return rows && in[i].publish ? h + trackbatch_down_at(o, i) + o.msg : (const char *)nullptr; };
  for (int i = 0; i < n; i++) {
    if (!trackbatch_active(in[i])) continue;
    const char *r = rows_at(i);
    if (!trackframe_counts_check(*(const TfDev *)(h + trackbatch_down_at(o, i) + o.dev), counts[i], MC, in[i].publish != 0, r ? *(const int *)r : 0)) {
      c->err = "lfvio_track_batch_frame: a count from the device beyond its bound";
      return LFVIO_ERR_DEVICE;
    }
  }
  for (int i = 0; i < n; i++) {
    if (!trackbatch_active(in[i])) {
      trackframe_zero(&out[i]);
      if (msg) msg[i].num_rows = 0;
      continue;
    }
    const char *dn = h + trackbatch_down_at(o, i);
    const TfDev *v = (const TfDev *)(dn + o.dev);
    trackframe_emit(TfDown{v, dn + o.table, shape.B_max, dn + o.un, dn + o.un3d, dn + o.vel, rows_at(i)}, LU, in[i].publish != 0, &out[i], msg ? &msg[i] : nullptr);
    b.slot[i].commit_frame(W, H, LU, v->num_points, v->num_new, in[i].time);
  }
  return LFVIO_OK;
}
