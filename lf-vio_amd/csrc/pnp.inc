// pnp.inc — host side of lfvio_pnp (include/lfvio.h): PnpSolver::compute_pose (pnp_solver.cpp) for F frames at once on
// k_pnp (kernels_pnp.h).  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate the CSR, pack [offset | point_w | bearing] into the staging block of feat.inc, one copy up, one
// launch (grid F), one copy down of the F records.

int lfvio_pnp(lfvio_ctx *c, const LfvioPnpIn *in, LfvioPnpOut *out) {
  static_assert(sizeof(PnpRecord) == sizeof(LfvioPnpOut), "the kernel writes LfvioPnpOut");
  if (!c || !in || !out) return LFVIO_ERR_ARG;
  const int F = in->num_frames;
  if (F < 1 || F > LFVIO_MAX_IMAGE_FRAMES || !in->offset || !in->point_w || !in->bearing) {
    c->err = "lfvio_pnp: num_frames outside [1, LFVIO_MAX_IMAGE_FRAMES] or null arrays";
    return LFVIO_ERR_ARG;
  }
  if (in->offset[0] != 0) {
    c->err = "lfvio_pnp: offset[0] != 0";
    return LFVIO_ERR_ARG;
  }
  for (int f = 0; f < F; f++) {
    const long long n = (long long)in->offset[f + 1] - in->offset[f];
    if (n < PNP_MIN_POINTS || n > PNP_MAX_POINTS) {
      c->err = "lfvio_pnp: a frame with fewer than 6 or more than 4096 correspondences (or offset not ascending)";
      return LFVIO_ERR_ARG;
    }
  }
  const size_t M = (size_t)in->offset[F];
  FeatStage st(c);
  const size_t oF = st.take((size_t)(F + 1) * 4), oP = st.take(M * 24), oU = st.take(M * 24), in_end = st.end;
  const size_t oA = st.take(M * 32), oO = st.take((size_t)F * sizeof(LfvioPnpOut));
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oF, in->offset, (size_t)(F + 1) * 4);
  std::memcpy(h + oP, in->point_w, M * 24);
  std::memcpy(h + oU, in->bearing, M * 24);
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_pnp, dim3(F), dim3(PNP_THREADS), 0, st.fs, (const int *)(d + oF), (const double *)(d + oP), (const double *)(d + oU),
                     (double *)(d + oA), (PnpRecord *)(d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, st.end)) return rc;
  const LfvioPnpOut *o = (const LfvioPnpOut *)(h + oO);
  for (int f = 0; f < F; f++) {
    if (o[f].status == 0)
      out[f] = o[f];
    else  // a non-finite value: R, T, err and chosen stay as the caller had them
      out[f].status = o[f].status;
  }
  return LFVIO_OK;
}
