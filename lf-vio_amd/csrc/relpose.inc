// relpose.inc — host side of lfvio_relative_pose (include/lfvio.h): Estimator::relativePose (estimator.cpp:445-473) over
// solveRelativeRT (initial/solve_5pts.cpp:536-576) on the kernels of kernels_relpose.h.  Included by lfvio_hip.hip inside its
// extern "C" block.
//
// One call: validate, pack [CSR | bearings | sample sets | zeroed records] into the staging block of feat.inc, one copy up, k_rp_hyp
// (grid (S + 1, P)), k_rp_fit (grid P), one copy down of [records | masks]; l is picked here from the P records.

int lfvio_relative_pose(lfvio_ctx *c, const LfvioRelativePoseIn *in, unsigned char *inlier, LfvioRelativePoseOut *out) {
  if (!c || !in || !out) return LFVIO_ERR_ARG;
  const int P = in->num_pairs, S = in->num_samples;
  if (P < 1 || P > LFVIO_WINDOW_SIZE || S < 1 || S > TV_MAX_SAMPLES || !in->match_offset || !in->bearing_l || !in->bearing_r || !in->samples) {
    c->err = "lfvio_relative_pose: num_pairs outside [1, LFVIO_WINDOW_SIZE], num_samples outside [1, 1024] or null arrays";
    return LFVIO_ERR_ARG;
  }
  const int *off = in->match_offset;
  if (off[0] != 0) {
    c->err = "lfvio_relative_pose: match_offset[0] != 0";
    return LFVIO_ERR_ARG;
  }
  for (int p = 0; p < P; p++) {
    const int N = off[p + 1] - off[p];
    if (N < 0 || N > TV_MAX_MATCHES) {
      c->err = "lfvio_relative_pose: a descending match_offset or a pair with more than 4096 matches";
      return LFVIO_ERR_ARG;
    }
    if (N <= RP_MIN_MATCHES) continue;  // its sample slots are never read
    const int *s = in->samples + (size_t)p * S * 8;
    for (int k = 0; k < 8 * S; k++)
      if (s[k] < 0 || s[k] >= N) {
        c->err = "lfvio_relative_pose: sample index outside [0, N_p)";
        return LFVIO_ERR_ARG;
      }
  }
  const size_t M = (size_t)off[P], PS = (size_t)P * S;
  FeatStage st(c);
  const size_t oF = st.take((size_t)(P + 1) * 4), oL = st.take(M * 24), oR = st.take(M * 24), oS = st.take(PS * 32);
  const size_t oO = st.take((size_t)P * sizeof(LfvioRelativePosePair)), in_end = st.end;
  const size_t oM = st.take(M), out_end = st.end;
  const size_t oG = st.take((size_t)P * 4), oC = st.take(PS * 4), oE = st.take(PS * 72), oA = st.take((M + 9 * (size_t)P) * 72);
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oF, off, (size_t)(P + 1) * 4);
  std::memcpy(h + oL, in->bearing_l, M * 24);
  std::memcpy(h + oR, in->bearing_r, M * 24);
  for (int p = 0; p < P; p++) {  // (the slots of a pair that is skipped may hold anything: they travel as zeros)
    const size_t o = (size_t)p * S * 32;
    if (off[p + 1] - off[p] > RP_MIN_MATCHES)
      std::memcpy(h + oS + o, in->samples + (size_t)p * S * 8, (size_t)S * 32);
    else
      std::memset(h + oS + o, 0, (size_t)S * 32);
  }
  {
    LfvioRelativePosePair *r = (LfvioRelativePosePair *)(h + oO);
    std::memset(r, 0, (size_t)P * sizeof *r);
    for (int p = 0; p < P; p++) r[p].best_sample = -1, r[p].chosen = -1;
  }
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_rp_hyp, dim3(S + 1, P), dim3(TV_HYP_THREADS), 0, st.fs, S, (const int *)(d + oF), (const double *)(d + oL),
                     (const double *)(d + oR), (const int *)(d + oS), (double *)(d + oE), (float *)(d + oC), (int *)(d + oG),
                     (LfvioRelativePosePair *)(d + oO));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_rp_fit, dim3(P), dim3(TV_FIT_THREADS), 0, st.fs, S, (const int *)(d + oF), (const double *)(d + oL),
                     (const double *)(d + oR), (const double *)(d + oE), (const float *)(d + oC), (const int *)(d + oG), (double *)(d + oA),
                     (unsigned char *)(d + oM), (LfvioRelativePosePair *)(d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, inlier ? out_end : in_end)) return rc;
  const LfvioRelativePosePair *r = (const LfvioRelativePosePair *)(h + oO);
  int l = -1;
  for (int p = 0; p < P; p++) {
    out->pair[p] = r[p];
    if (inlier && r[p].gate == 0) std::memcpy(inlier + off[p], h + oM + off[p], (size_t)(off[p + 1] - off[p]));
    if (l < 0 && r[p].gate == 0 && r[p].ok) l = p;
  }
  out->l = l, out->pad_ = 0;
  if (l >= 0) {
    std::memcpy(out->relative_R, r[l].rotation, sizeof out->relative_R);
    std::memcpy(out->relative_T, r[l].translation, sizeof out->relative_T);
  }
  return LFVIO_OK;
}
