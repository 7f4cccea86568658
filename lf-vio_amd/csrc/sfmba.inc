// sfmba.inc — host side of lfvio_sfm_ba (include/lfvio.h): the full BA of GlobalSFM::construct (initial_sfm.cpp:233-309) on k_sfm_ba
// (kernels_sfmba.h).  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate the CSR, build the (point, frame) -> observation table, pack [head | CSR | table | bearings | state | record]
// into the staging block of feat.inc, one copy up, one launch (one workgroup runs the whole loop), one copy down of the state and
// the record.  The kernel's per-point and per-observation blocks live behind the record and never cross the bus.

int lfvio_sfm_ba(lfvio_ctx *c, const LfvioSfmBaIn *in, double *c_rotation, double *c_translation, double *position, LfvioSfmBaOut *out) {
  if (!c || !in || !out || !c_rotation || !c_translation || !position) return LFVIO_ERR_ARG;
  const int F = in->num_frames, l = in->ref_frame, P = in->num_points;
  if (F < 2 || F > LFVIO_NUM_FRAMES || l < 0 || l > F - 2 || P < 1 || P > SFMBA_MAX_POINTS || !in->obs_offset || !in->obs_frame || !in->obs_bearing ||
      in->max_num_iterations > LFVIO_MAX_TRACE - 1) {
    c->err = "lfvio_sfm_ba: num_frames outside [2, LFVIO_NUM_FRAMES], ref_frame outside [0, F - 2], num_points outside [1, 4096], null arrays or more than LFVIO_MAX_TRACE - 1 iterations";
    return LFVIO_ERR_ARG;
  }
  if (in->obs_offset[0] != 0) {
    c->err = "lfvio_sfm_ba: obs_offset[0] != 0";
    return LFVIO_ERR_ARG;
  }
  for (int i = 0; i < P; i++) {
    const long long k = (long long)in->obs_offset[i + 1] - in->obs_offset[i];
    if (k < 1 || k > F) {
      c->err = "lfvio_sfm_ba: a point with no observation or more than num_frames (or obs_offset not ascending)";
      return LFVIO_ERR_ARG;
    }
  }
  const size_t M = (size_t)in->obs_offset[P];
  std::vector<int> slot((size_t)P * F, -1);
  for (int i = 0; i < P; i++)
    for (int o = in->obs_offset[i]; o < in->obs_offset[i + 1]; o++) {
      const int f = in->obs_frame[o];
      if (f < 0 || f >= F || slot[(size_t)i * F + f] >= 0) {
        c->err = "lfvio_sfm_ba: an obs_frame outside [0, num_frames) or a frame listed twice for one point";
        return LFVIO_ERR_ARG;
      }
      slot[(size_t)i * F + f] = o;
    }
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
