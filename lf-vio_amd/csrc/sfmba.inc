// sfmba.inc — host side of lfvio_sfm_ba (include/lfvio.h): the full BA of GlobalSFM::construct (initial_sfm.cpp:233-309) on k_sfm_ba
// (kernels_sfmba.h).  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate the CSR, build the (point, frame) -> observation table, pack [head | CSR | table | bearings | state | record]
// into the staging block of feat.inc, one copy up, one launch (one workgroup runs the whole loop), one copy down of the state and
// the record.  The kernel's per-point and per-observation blocks live behind the record and never cross the bus.

// The CSR checks that lfvio_sfm_ba and lfvio_sfm_construct (sfmchain.inc) share, and the (point, frame) -> observation table both
// kernels walk.  Returns 0, or the check that failed: 1 obs_offset[0] != 0; 2 a point with no observation or more than F (which covers
// an offset array that is not ascending); 3 an obs_frame outside [0, F) or a frame listed twice for one point.
static int sfm_obs_table(int F, int P, const int *obs_offset, const int *obs_frame, std::vector<int> &slot) {
  if (obs_offset[0] != 0) return 1;
  for (int i = 0; i < P; i++) {
    const long long k = (long long)obs_offset[i + 1] - obs_offset[i];
    if (k < 1 || k > F) return 2;
  }
  slot.assign((size_t)P * F, -1);
  for (int i = 0; i < P; i++)
    for (int o = obs_offset[i]; o < obs_offset[i + 1]; o++) {
      const int f = obs_frame[o];
      if (f < 0 || f >= F || slot[(size_t)i * F + f] >= 0) return 3;
      slot[(size_t)i * F + f] = o;
    }
  return 0;
}

int lfvio_sfm_ba(lfvio_ctx *c, const LfvioSfmBaIn *in, double *c_rotation, double *c_translation, double *position, LfvioSfmBaOut *out) {
  if (!c || !in || !out || !c_rotation || !c_translation || !position) return LFVIO_ERR_ARG;
  const int F = in->num_frames, l = in->ref_frame, P = in->num_points;
  if (F < 2 || F > LFVIO_NUM_FRAMES || l < 0 || l > F - 2 || P < 1 || P > SFMBA_MAX_POINTS || !in->obs_offset || !in->obs_frame || !in->obs_bearing ||
      in->max_num_iterations > LFVIO_MAX_TRACE - 1) {
    c->err = "lfvio_sfm_ba: num_frames outside [2, LFVIO_NUM_FRAMES], ref_frame outside [0, F - 2], num_points outside [1, 4096], null arrays or more than LFVIO_MAX_TRACE - 1 iterations";
    return LFVIO_ERR_ARG;
  }
  std::vector<int> slot;
  if (const int bad = sfm_obs_table(F, P, in->obs_offset, in->obs_frame, slot)) {
    c->err = bad == 1   ? "lfvio_sfm_ba: obs_offset[0] != 0"
             : bad == 2 ? "lfvio_sfm_ba: a point with no observation or more than num_frames (or obs_offset not ascending)"
                        : "lfvio_sfm_ba: an obs_frame outside [0, num_frames) or a frame listed twice for one point";
    return LFVIO_ERR_ARG;
  }
  const size_t M = (size_t)in->obs_offset[P];
  SfmBaHead hd;
  std::memset(&hd, 0, sizeof hd);
  hd.F = F, hd.P = P;
  hd.max_it = in->max_num_iterations < 0 ? 50 : in->max_num_iterations;
  hd.ftol = in->function_tolerance > 0 ? in->function_tolerance : 1e-6;
  hd.gtol = in->gradient_tolerance > 0 ? in->gradient_tolerance : 1e-10;
  hd.ptol = in->parameter_tolerance > 0 ? in->parameter_tolerance : 1e-8;
  int n = 0;
  for (int f = 0; f < LFVIO_NUM_FRAMES; f++)
    for (int k = 0; k < 6; k++) {
      const bool free_col = f < F && f != l && (k < 3 || f != F - 1);  // rotation of l; translations of l and F - 1 (:249-256)
      hd.col[f][k] = free_col ? n++ : -1;
    }
  hd.n = n;  // 6 F - 9

  FeatStage st(c);
  const size_t oH = st.take(sizeof hd), oF = st.take((size_t)(P + 1) * 4), oM = st.take(M * 4), oS = st.take((size_t)P * F * 4), oB = st.take(M * 24);
  const size_t oQ = st.take((size_t)F * 32), oT = st.take((size_t)F * 24), oX = st.take((size_t)P * 24), oR = st.take(sizeof(SfmBaResult)), io_end = st.end;
  const size_t oXc = st.take((size_t)P * 24), oPw = st.take((size_t)P * SFMBA_PW * 8), oOw = st.take(M * SFMBA_OW * 8);
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oH, &hd, sizeof hd);
  std::memcpy(h + oF, in->obs_offset, (size_t)(P + 1) * 4);
  std::memcpy(h + oM, in->obs_frame, M * 4);
  std::memcpy(h + oS, slot.data(), (size_t)P * F * 4);
  std::memcpy(h + oB, in->obs_bearing, M * 24);
  std::memcpy(h + oQ, c_rotation, (size_t)F * 32);
  std::memcpy(h + oT, c_translation, (size_t)F * 24);
  std::memcpy(h + oX, position, (size_t)P * 24);
  std::memset(h + oR, 0, sizeof(SfmBaResult));
  if (int rc = st.up(io_end)) return rc;
  hipLaunchKernelGGL(k_sfm_ba, dim3(1), dim3(SFMBA_THREADS), 0, st.fs, (const SfmBaHead *)(d + oH), (const int *)(d + oF), (const int *)(d + oM),
                     (const int *)(d + oS), (const double *)(d + oB), (double *)(d + oQ), (double *)(d + oT), (double *)(d + oX), (double *)(d + oXc),
                     (double *)(d + oPw), (double *)(d + oOw), (SfmBaResult *)(d + oR));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oQ, io_end)) return rc;
  const SfmBaResult *r = (const SfmBaResult *)(h + oR);
  if (r->nonfinite) {
    c->err = "lfvio_sfm_ba: non-finite initial cost";
    return LFVIO_ERR_NONFINITE;
  }
  std::memcpy(c_rotation, h + oQ, (size_t)F * 32);
  std::memcpy(c_translation, h + oT, (size_t)F * 24);
  std::memcpy(position, h + oX, (size_t)P * 24);
  out->termination = r->o.termination, out->num_iterations = r->o.num_iterations;
  out->num_successful_steps = r->o.num_successful_steps, out->num_unsuccessful_steps = r->o.num_unsuccessful_steps;
  out->accepted = r->o.accepted, out->pad_ = 0, out->initial_cost = r->o.initial_cost, out->final_cost = r->o.final_cost;
  std::memcpy(out->Q, r->o.Q, (size_t)F * 32);
  std::memcpy(out->T, r->o.T, (size_t)F * 24);
  std::memcpy(out->trace, r->o.trace, sizeof out->trace);
  return LFVIO_OK;
}
