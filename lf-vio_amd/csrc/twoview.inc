// twoview.inc — host side of lfvio_two_view (include/lfvio.h): the two-view RANSAC of InitialEXRotation::solveRelativeR
// (initial/initial_ex_rotation.cpp:157-284) on the kernels of kernels_twoview.h.  Included by lfvio_hip.hip inside its
// extern "C" block.
//
// One call: validate, pack bearings and sample sets into the staging block of feat.inc, one copy up, k_tv_hyp (grid S),
// k_tv_fit (one workgroup), one copy down of [LfvioTwoViewOut | mask | scores | hypotheses] as far as the caller asked.

int lfvio_two_view(lfvio_ctx *c, const LfvioTwoViewIn *in, unsigned char *inlier, LfvioTwoViewOut *out, double *E_all, float *score_all) {
  if (!c || !in || !inlier || !out) return LFVIO_ERR_ARG;
  const int N = in->num_matches, S = in->num_samples;
  if (N < 8 || N > TV_MAX_MATCHES || S < 1 || S > TV_MAX_SAMPLES || !in->bearing_l || !in->bearing_r || !in->samples) {
    c->err = "lfvio_two_view: num_matches outside [8, 4096], num_samples outside [1, 1024] or null arrays";
    return LFVIO_ERR_ARG;
  }
  for (int k = 0; k < 8 * S; k++)
    if (in->samples[k] < 0 || in->samples[k] >= N) {
      c->err = "lfvio_two_view: sample index outside [0, num_matches)";
      return LFVIO_ERR_ARG;
    }
  FeatStage st(c);
  const size_t NR = (size_t)std::max(N, 9);
  const size_t oL = st.take((size_t)N * 24), oR = st.take((size_t)N * 24), oS = st.take((size_t)S * 32), in_end = st.end;
  const size_t oA = st.take(NR * 72), oO = st.take(sizeof(LfvioTwoViewOut)), oM = st.take((size_t)N), oC = st.take((size_t)S * 4),
               oE = st.take((size_t)S * 72);
  if (int rc = st.reserve()) return rc;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oL, in->bearing_l, (size_t)N * 24);
  std::memcpy(h + oR, in->bearing_r, (size_t)N * 24);
  std::memcpy(h + oS, in->samples, (size_t)S * 32);
  if (int rc = st.up(in_end)) return rc;
  hipLaunchKernelGGL(k_tv_hyp, dim3(S), dim3(TV_HYP_THREADS), 0, st.fs, N, (const double *)(d + oL), (const double *)(d + oR),
                     (const int *)(d + oS), (double *)(d + oE), (float *)(d + oC));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_tv_fit, dim3(1), dim3(TV_FIT_THREADS), 0, st.fs, N, S, (const double *)(d + oL), (const double *)(d + oR),
                     (const double *)(d + oE), (const float *)(d + oC), (double *)(d + oA), (unsigned char *)(d + oM),
                     (LfvioTwoViewOut *)(d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, E_all ? st.end : score_all ? oC + (size_t)S * 4 : oM + (size_t)N)) return rc;
  const LfvioTwoViewOut *o = (const LfvioTwoViewOut *)(h + oO);
  if (o->status == 0) {
    *out = *o;
    std::memcpy(inlier, h + oM, (size_t)N);
  } else {  // no model: E, the candidates, front, R_rel and the mask stay as the caller had them
    out->status = o->status, out->best_sample = o->best_sample, out->num_inliers = o->num_inliers, out->best_score = o->best_score;
  }
  if (E_all) std::memcpy(E_all, h + oE, (size_t)S * 72);
  if (score_all) std::memcpy(score_all, h + oC, (size_t)S * 4);
  return LFVIO_OK;
}
