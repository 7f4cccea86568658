// vialign.inc — host side of lfvio_vi_align (include/lfvio.h): VisualIMUAlignment (initial/initial_aligment.cpp:3-216) on the
// kernels of kernels_vialign.h and the existing k_preintegrate.  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate, pack [ImuJobs | noise | samples | R | T | tic, G] into the staging block of feat.inc, one copy up,
//   k_preintegrate (the spans as passed) -> k_va_bias (delta_bg; writes ba = 0, bg = Bgs[0] + delta_bg into the jobs on the device)
//   -> k_preintegrate (the same launch again) -> k_va_align (LinearAlignment + RefineGravity)
// and one copy down of [LfvioViAlignOut | x | pre] as far as the caller asked.  No host round trip in between.

int lfvio_vi_align(lfvio_ctx *c, const LfvioViAlignIn *in, LfvioViAlignOut *out, double *x, LfvioPreintegration *pre) {
  if (!c || !in || !out || !x) return LFVIO_ERR_ARG;
  const int F = in->num_frames;
  if (F < 4 || F > LFVIO_MAX_IMAGE_FRAMES || !in->R || !in->T || !in->span) {
    c->err = "lfvio_vi_align: num_frames outside [4, 128] or null arrays";
    return LFVIO_ERR_ARG;
  }
  size_t S = 0;
  for (int k = 1; k < F; k++) {
    const LfvioImuInterval &sp = in->span[k];
    if (sp.num_samples <= 0 || !sp.dt || !sp.acc || !sp.gyr) {
      c->err = "lfvio_vi_align: span without samples or with null sample arrays";
      return LFVIO_ERR_ARG;
    }
    double sum_dt = 0.0;
    for (int s = 0; s < sp.num_samples; s++) sum_dt += sp.dt[s];
    if (sum_dt == 0.0) {
      c->err = "lfvio_vi_align: span with sum_dt == 0";
      return LFVIO_ERR_ARG;
    }
    S += (size_t)sp.num_samples;
  }
  FeatStage st(c);
  const size_t K = (size_t)F - 1;
  const ImuStage im = imu_take(st, K, S);
  const size_t oR = st.take((size_t)F * 72), oP = st.take((size_t)F * 24), oV = st.take(sizeof(VaParams)), in_end = st.end;
  const size_t oO = st.take(sizeof(LfvioViAlignOut)), oX = st.take((size_t)F * 24), oI = st.take(K * sizeof(LfvioPreintegration));
  if (int rc = st.reserve()) return rc;
  char *h = st.h, *d = st.d;
  imu_pack(h, im, (int)K, in->span + 1, in->noise);
  std::memcpy(h + oR, in->R, (size_t)F * 72);
  std::memcpy(h + oP, in->T, (size_t)F * 24);
  VaParams prm;
  std::memcpy(prm.tic, in->tic, 24), prm.g_norm = in->g_norm;
  std::memcpy(h + oV, &prm, sizeof prm);
  if (int rc = st.up(in_end)) return rc;
  ImuJob *jobs = (ImuJob *)(d + im.jobs);
  LfvioPreintegration *dpre = (LfvioPreintegration *)(d + oI);
  LfvioViAlignOut *dout = (LfvioViAlignOut *)(d + oO);
  for (int pass = 0; pass < 2; pass++) {
    hipLaunchKernelGGL(k_preintegrate, dim3((unsigned)K), dim3(PRE_THREADS), 0, st.fs, (const ImuJob *)jobs, (const double *)(d + im.dt),
                       (const double *)(d + im.acc), (const double *)(d + im.gyr), (const double *)(d + im.noise), dpre);
    HIPCHK(c, hipGetLastError());
    if (pass == 0)
      hipLaunchKernelGGL(k_va_bias, dim3(1), dim3(VA_THREADS), 0, st.fs, F, (const double *)(d + oR), (const LfvioPreintegration *)dpre, jobs, dout);
    else
      hipLaunchKernelGGL(k_va_align, dim3(1), dim3(VA_THREADS), 0, st.fs, F, (const double *)(d + oR), (const double *)(d + oP),
                         (const LfvioPreintegration *)dpre, (const VaParams *)(d + oV), dout, (double *)(d + oX));
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.down(oO, pre ? st.end : oI)) return rc;
  const LfvioViAlignOut *o = (const LfvioViAlignOut *)(h + oO);
  if (o->status == 0) {
    *out = *o;
    std::memcpy(x, h + oX, (size_t)F * 24);
    if (pre) std::memcpy(pre + 1, h + oI, K * sizeof(LfvioPreintegration));
  } else if (o->status == 3) {  // a pivot that is not > 0: nothing but the status
    out->status = 3;
  } else {  // a gate of LinearAlignment: what the reference had computed by then (Bgs have moved, :28-29); x and pre stay
    const int st = o->status;
    out->status = st;
    std::memcpy(out->delta_bg, o->delta_bg, 24), std::memcpy(out->g_linear, o->g_linear, 24), out->s_linear = o->s_linear;
    if (st == 2) std::memcpy(out->g_iter, o->g_iter, sizeof o->g_iter), std::memcpy(out->g, o->g, 24), out->s = o->s;
  }
  return LFVIO_OK;
}
