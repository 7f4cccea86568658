// sfmchain.inc — host side of lfvio_sfm_construct (include/lfvio.h): the incremental part of GlobalSFM::construct
// (initial_sfm.cpp:121-218) on k_sfm_chain (kernels_sfmchain.h).  Included by lfvio_hip.hip inside its extern "C" block, after sfmba.inc,
// whose CSR check and (point, frame) -> observation table it shares.
//
// One call: validate, pack [head | CSR | table | bearings | record] into the staging block of feat.inc, one copy up, one launch (one
// workgroup runs the whole schedule), one copy down of [poses | positions | tri_op | record].  The gathered correspondences of a PnP
// and their barycentric coordinates live behind the record and never cross the bus.

int lfvio_sfm_construct(lfvio_ctx *c, const LfvioSfmConstructIn *in, double *c_rotation, double *c_translation, double *position, int *tri_op,
                        LfvioSfmConstructOut *out) {
  static_assert(sizeof(PnpRecord) == sizeof(LfvioPnpOut), "the kernel writes LfvioPnpOut");
  if (!c || !in || !out || !c_rotation || !c_translation || !position || !tri_op) return LFVIO_ERR_ARG;
  const int F = in->num_frames, l = in->ref_frame, P = in->num_points;
  if (F < 2 || F > LFVIO_NUM_FRAMES || l < 0 || l > F - 2 || P < 1 || P > SFMCH_MAX_POINTS || !in->obs_offset || !in->obs_frame || !in->obs_bearing) {
    c->err = "lfvio_sfm_construct: num_frames outside [2, LFVIO_NUM_FRAMES], ref_frame outside [0, F - 2], num_points outside [1, 4096] or null arrays";
    return LFVIO_ERR_ARG;
  }
  std::vector<int> slot;
  if (const int bad = sfm_obs_table(F, P, in->obs_offset, in->obs_frame, slot)) {
    c->err = bad == 1   ? "lfvio_sfm_construct: obs_offset[0] != 0"
             : bad == 2 ? "lfvio_sfm_construct: a point with no observation or more than num_frames (or obs_offset not ascending)"
                        : "lfvio_sfm_construct: an obs_frame outside [0, num_frames) or a frame listed twice for one point";
    return LFVIO_ERR_ARG;
  }
  const size_t M = (size_t)in->obs_offset[P];
  SfmChainHead hd;
  std::memset(&hd, 0, sizeof hd);
  hd.F = F, hd.l = l, hd.P = P;
  std::memcpy(hd.relative_R, in->relative_R, sizeof hd.relative_R);
  std::memcpy(hd.relative_T, in->relative_T, sizeof hd.relative_T);

  FeatStage st(c);
  const size_t oH = st.take(sizeof hd), oF = st.take((size_t)(P + 1) * 4), oM = st.take(M * 4), oS = st.take((size_t)P * F * 4), oB = st.take(M * 24);
  const size_t oR = st.take(sizeof(SfmChainResult)), in_end = st.end;
  const size_t oQ = st.take((size_t)F * 32), oT = st.take((size_t)F * 24), oX = st.take((size_t)P * 24), oO = st.take((size_t)P * 4), out_end = st.end;
  const size_t oGp = st.take((size_t)P * 24), oGu = st.take((size_t)P * 24), oGa = st.take((size_t)P * 32);
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oH, &hd, sizeof hd);
  std::memcpy(h + oF, in->obs_offset, (size_t)(P + 1) * 4);
  std::memcpy(h + oM, in->obs_frame, M * 4);
  std::memcpy(h + oS, slot.data(), (size_t)P * F * 4);
  std::memcpy(h + oB, in->obs_bearing, M * 24);
  {
    SfmChainResult *r = (SfmChainResult *)(h + oR);
    std::memset(r, 0, sizeof *r);
    r->o.failed_frame = -1;
    for (int f = 0; f < LFVIO_NUM_FRAMES; f++) r->o.pnp_op[f] = -1;
  }
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_sfm_chain, dim3(1), dim3(SFMCH_THREADS), 0, st.fs, (const SfmChainHead *)(d + oH), (const int *)(d + oF), (const int *)(d + oM),
                     (const int *)(d + oS), (const double *)(d + oB), (double *)(d + oQ), (double *)(d + oT), (double *)(d + oX), (int *)(d + oO),
                     (double *)(d + oGp), (double *)(d + oGu), (double *)(d + oGa), (SfmChainResult *)(d + oR));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oR, out_end)) return rc;
  const SfmChainResult *r = (const SfmChainResult *)(h + oR);
  for (int f = 0; f < F; f++)
    if (r->posed[f]) {  // a frame the chain did not reach keeps the caller's rows
      std::memcpy(c_rotation + 4 * f, h + oQ + (size_t)f * 32, 32);
      std::memcpy(c_translation + 3 * f, h + oT + (size_t)f * 24, 24);
    }
  std::memcpy(position, h + oX, (size_t)P * 24);
  std::memcpy(tri_op, h + oO, (size_t)P * 4);
  *out = r->o;
  int nt = 0;
  for (int j = 0; j < P; j++) nt += tri_op[j] >= 0 ? 1 : 0;
  out->num_triangulated = nt, out->pad_ = 0;
  return LFVIO_OK;
}
