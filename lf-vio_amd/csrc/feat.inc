// feat.inc — the calls on the feature stream (include/lfvio.h): their shared staging, and lfvio_triangulate,
// lfvio_shift_depth and lfvio_preintegrate on the kernels of kernels_feat.h (SURVEY §8f ranks 2 and 3).  Included by
// lfvio_hip.hip inside its extern "C" block; twoview.inc, vialign.inc and pnp.inc stage the same way.
//
// One call: validate, pack the inputs into the pinned staging block, one copy up, the launches, one copy down.  (A copy from
// pageable memory costs ~20 us each on this runtime: one packed pinned block instead of one copy per array.)

static int feat_reserve(lfvio_ctx *c, size_t bytes) {
  if (bytes <= c->h_feat.capacity()) return LFVIO_OK;  // (the two halves have one size, or are both empty)
  (void)c->d_feat.reset(), (void)c->h_feat.reset();
  bytes = align_up(bytes + bytes / 4, 4096);
  if (!c->d_feat.reserve(bytes) || !c->h_feat.reserve(bytes)) {
    (void)c->d_feat.reset();
    return out_of_memory(c, "out of memory (feature scratch)");
  }
  return LFVIO_OK;
}

// The staging block of one call: take() the segments in order, reserve(), fill h, up(), launch on fs, down().
struct FeatStage {
  lfvio_ctx *c;
  hipStream_t fs;
  size_t end = 0;  // of the last segment taken
  char *h = nullptr, *d = nullptr;
  explicit FeatStage(lfvio_ctx *ctx) : c(ctx) {
    (void)hipSetDevice(c->device);
    fs = c->fstream ? c->fstream : c->stream;  // not behind the tail of an optimization still in flight
  }
  size_t take(size_t bytes) {  // a 256-aligned offset
    const size_t o = align_up(end, 256);
    end = o + bytes;
    return o;
  }
  int reserve() {
    int rc = feat_reserve(c, end);
    h = c->h_feat, d = c->d_feat;
    return rc;
  }
  int up(size_t in_end) {
    HIPCHK(c, hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, fs));
    return LFVIO_OK;
  }
  int down(size_t from, size_t to) {  // and wait for it
    HIPCHK(c, hipMemcpyAsync(h + from, d + from, to - from, hipMemcpyDeviceToHost, fs));
    HIPCHK(c, hipStreamSynchronize(fs));
    return LFVIO_OK;
  }
};

// K ImuJobs, the noise and S samples: the inputs of k_preintegrate
struct ImuStage {
  size_t jobs, noise, dt, acc, gyr;
};
static ImuStage imu_take(FeatStage &st, size_t K, size_t S) {
  ImuStage o;
  o.jobs = st.take(K * sizeof(ImuJob)), o.noise = st.take(32), o.dt = st.take(S * 8), o.acc = st.take(S * 24), o.gyr = st.take(S * 24);
  return o;
}
static void imu_pack(char *h, const ImuStage &o, int K, const LfvioImuInterval *in, const double noise[4]) {
  size_t off = 0;
  for (int k = 0; k < K; k++) {
    ImuJob *jb = (ImuJob *)(h + o.jobs) + k;
    const size_t n = (size_t)in[k].num_samples;
    jb->n = (int)n, jb->off = (int)off;
    std::memcpy(jb->acc_0, in[k].acc_0, 24), std::memcpy(jb->gyr_0, in[k].gyr_0, 24);
    std::memcpy(jb->ba, in[k].linearized_ba, 24), std::memcpy(jb->bg, in[k].linearized_bg, 24);
    if (n) {
      std::memcpy(h + o.dt + off * 8, in[k].dt, n * 8);
      std::memcpy(h + o.acc + off * 24, in[k].acc, n * 24);
      std::memcpy(h + o.gyr + off * 24, in[k].gyr, n * 24);
    }
    off += n;
  }
  std::memcpy(h + o.noise, noise, 32);
}

int lfvio_triangulate(lfvio_ctx *c, const LfvioTriangulateIn *in, double *estimated_depth) {
  if (!c || !in || in->num_landmarks < 0 || in->num_observations < 0) return LFVIO_ERR_ARG;
  const int N = in->num_landmarks, M = in->num_observations;
  if (N == 0) return LFVIO_OK;
  if (!estimated_depth || !in->start_frame || !in->obs_offset || !in->obs_point || in->obs_offset[0] != 0 || in->obs_offset[N] != M) {
    c->err = "triangulate: null arrays or obs_offset is not a CSR over num_observations";
    return LFVIO_ERR_ARG;
  }
  for (int l = 0; l < N; l++) {
    const int k = in->obs_offset[l + 1] - in->obs_offset[l], s = in->start_frame[l];
    if (k < 2 || s < 0 || s + k > LFVIO_NUM_FRAMES) {
      c->err = "triangulate: landmark with fewer than 2 observations or a track leaving the window";
      return LFVIO_ERR_ARG;
    }
  }
  FeatStage st(c);
  const size_t oF = st.take(sizeof(FeatFrames)), oS = st.take((size_t)N * 4), oO = st.take((size_t)(N + 1) * 4), oP = st.take((size_t)M * 24),
               oD = st.take((size_t)N * 8);
  if (int rc = st.reserve()) return rc;
  FeatFrames F;
  std::memcpy(F.Ps, in->Ps, sizeof F.Ps), std::memcpy(F.Rs, in->Rs, sizeof F.Rs);
  std::memcpy(F.tic, in->tic, sizeof F.tic), std::memcpy(F.ric, in->ric, sizeof F.ric);
  F.init_depth = in->init_depth;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oF, &F, sizeof F);
  std::memcpy(h + oS, in->start_frame, (size_t)N * 4);
  std::memcpy(h + oO, in->obs_offset, (size_t)(N + 1) * 4);
  std::memcpy(h + oP, in->obs_point, (size_t)M * 24);
  std::memcpy(h + oD, estimated_depth, (size_t)N * 8);
  if (int rc = st.up(st.end)) return rc;
  hipLaunchKernelGGL(k_triangulate, dim3((N + TRI_THREADS - 1) / TRI_THREADS), dim3(TRI_THREADS), 0, st.fs, (const FeatFrames *)(d + oF), N,
                     (const int *)(d + oS), (const int *)(d + oO), (const double *)(d + oP), (double *)(d + oD));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oD, st.end)) return rc;
  std::memcpy(estimated_depth, h + oD, (size_t)N * 8);
  return LFVIO_OK;
}

int lfvio_shift_depth(lfvio_ctx *c, int n, const double *uv_i, const double marg_R[9], const double marg_P[3], const double new_R[9],
                      const double new_P[3], double init_depth, double *estimated_depth) {
  if (!c || n < 0) return LFVIO_ERR_ARG;
  if (n == 0) return LFVIO_OK;
  if (!uv_i || !marg_R || !marg_P || !new_R || !new_P || !estimated_depth) return LFVIO_ERR_ARG;
  FeatStage st(c);
  double T[25];
  const size_t oT = st.take(sizeof T), oU = st.take((size_t)n * 24), oD = st.take((size_t)n * 8);
  if (int rc = st.reserve()) return rc;
  std::memcpy(T, marg_R, 72), std::memcpy(T + 9, marg_P, 24), std::memcpy(T + 12, new_R, 72), std::memcpy(T + 21, new_P, 24);
  T[24] = init_depth;
  char *d = st.d, *h = st.h;
  std::memcpy(h + oT, T, sizeof T);
  std::memcpy(h + oU, uv_i, (size_t)n * 24);
  std::memcpy(h + oD, estimated_depth, (size_t)n * 8);
  if (int rc = st.up(st.end)) return rc;
  hipLaunchKernelGGL(k_shift_depth, dim3((n + 255) / 256), dim3(256), 0, st.fs, n, (const double *)(d + oU), (const double *)(d + oT),
                     (double *)(d + oD));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oD, st.end)) return rc;
  std::memcpy(estimated_depth, h + oD, (size_t)n * 8);
  return LFVIO_OK;
}

int lfvio_preintegrate(lfvio_ctx *c, int num_intervals, const LfvioImuInterval *in, const double noise[4], LfvioPreintegration *out) {
  if (!c || num_intervals < 0) return LFVIO_ERR_ARG;
  if (num_intervals == 0) return LFVIO_OK;
  if (!in || !noise || !out) return LFVIO_ERR_ARG;
  size_t S = 0;
  for (int k = 0; k < num_intervals; k++) {
    if (in[k].num_samples < 0 || (in[k].num_samples > 0 && (!in[k].dt || !in[k].acc || !in[k].gyr))) {
      c->err = "preintegrate: interval with a negative sample count or null sample arrays";
      return LFVIO_ERR_ARG;
    }
    S += (size_t)in[k].num_samples;
  }
  FeatStage st(c);
  const size_t K = (size_t)num_intervals;
  const ImuStage im = imu_take(st, K, S);
  const size_t oO = st.take(K * sizeof(LfvioPreintegration));
  if (int rc = st.reserve()) return rc;
  imu_pack(st.h, im, num_intervals, in, noise);
  char *d = st.d;
  if (int rc = st.up(oO)) return rc;
  hipLaunchKernelGGL(k_preintegrate, dim3(num_intervals), dim3(PRE_THREADS), 0, st.fs, (const ImuJob *)(d + im.jobs), (const double *)(d + im.dt),
                     (const double *)(d + im.acc), (const double *)(d + im.gyr), (const double *)(d + im.noise), (LfvioPreintegration *)(d + oO));
  HIPCHK(c, hipGetLastError());
  if (int rc = st.down(oO, st.end)) return rc;
  std::memcpy(out, st.h + oO, K * sizeof(LfvioPreintegration));
  return LFVIO_OK;
}
