// relo.inc — host side of lfvio_solve_relo (include/lfvio.h): the relocalization branch of Estimator::optimization()
// (estimator.cpp:777-808) on the route of kernels_relo.h.  Included by lfvio_hip.hip inside its extern "C" block.
//
// One call: validate, pack the window and the relo table into one pinned staging blob, one copy up, then one launch sequence
// per trust-region pass (k_relo_eval -> k_relo_gram -> k_relo_solve 0 -> k_relo_schur -> k_relo_solve 1 -> k_relo_eval<false>
// -> k_relo_decide; the first three return at once in a pass that does not linearize, the Schur kernel in a pass that reuses
// its Gauss-Newton step) and one 4-byte read of the loop's `done` word behind it.  A relo solve
// happens once per loop-closure message, so neither graph capture nor speculation is spent on it.

namespace {

int relo_refused(lfvio_ctx *c, int rc) {  // (the error text of a shared check, marked as this entry point's)
  c->err = "lfvio_solve_relo: " + c->err;
  return rc;
}

int relo_check(lfvio_ctx *c, const LfvioWindow *in, const LfvioRelo *relo) {
  auto bad = [&](const char *what) {
    c->err = std::string("lfvio_solve_relo: ") + what;
    return LFVIO_ERR_ARG;
  };
  if (int rc = check_window(c, in)) return relo_refused(c, rc);
  const int N = in->num_landmarks;
  const LfvioPrior *pr = (in->prior && in->prior->valid) ? in->prior : nullptr;
  if (int rc = check_input_prior(c, pr)) return rc;
  if (!relo) return bad("null relo");
  if (relo->frame < 0 || relo->frame >= LFVIO_WINDOW_SIZE) return bad("relo frame out of range");
  const int K = relo->num_matches;
  if (K < 0 || (K > 0 && (!relo->landmark || !relo->match_point))) return bad("num_matches < 0 or null match arrays");
  for (int k = 0; k < K; k++) {
    const int l = relo->landmark[k];
    if (l < 0 || l >= N) return bad("match landmark index out of range");
    if (k > 0 && l <= relo->landmark[k - 1]) return bad("match landmark indices not strictly ascending");
    if (in->start_frame[l] > relo->frame) return bad("matched landmark starts after the relo frame");
  }
  return LFVIO_OK;
}

struct ReloLayout {
  size_t start, off, rk, pt, vel, ctd, uvy, mp, lam0, pJ, pr, in_end;  // uploaded
  size_t lam0w, lam1w, J, gpart, Hs, Sg, gs, W, h, gl, lcost, scale_l, diag_l, gn_l, stp_l, hs, gsl, total;
};

ReloLayout relo_layout(int N, int M, int K, int R, int pn) {
  ReloLayout L;
  size_t o = align_up(sizeof(ReloDev), 256);
  auto take = [&](size_t bytes) {
    const size_t r = o;
    o = align_up(o + std::max<size_t>(bytes, 8), 256);
    return r;
  };
  const size_t n = std::max(N, 1), m = std::max(M, 1);
  L.start = take(n * 4), L.off = take((n + 1) * 4), L.rk = take(n * 4);
  L.pt = take(m * 24), L.vel = take(m * 24), L.ctd = take(m * 8), L.uvy = take(m * 8);
  L.mp = take((size_t)std::max(K, 1) * 16), L.lam0 = take(n * 8);
  L.pJ = take((size_t)pn * pn * 8), L.pr = take((size_t)pn * 8);
  L.in_end = o;
  L.lam0w = take(n * 8), L.lam1w = take(n * 8);
  L.J = take((size_t)R * RLD * 8);
  L.gpart = take((size_t)RELO_GCH * RG * RG * 8);
  L.Hs = take((size_t)RK * RK * 8), L.Sg = take((size_t)RK * (RK + 1) * 8), L.gs = take((size_t)RK * 8);
  L.W = take(n * RK * 8);
  L.h = take(n * 8), L.gl = take(n * 8), L.lcost = take(n * 8), L.scale_l = take(n * 8), L.diag_l = take(n * 8);
  L.gn_l = take(n * 8), L.stp_l = take(n * 8), L.hs = take(n * 8), L.gsl = take(n * 8);
  L.total = align_up(o, 4096);
  return L;
}

int relo_grow(lfvio_ctx *c, size_t dev_bytes, size_t stage_bytes) {
  MEMCHK(c, c->d_relo.reserve(dev_bytes), "hipMalloc((void **)&c->d_relo, dev_bytes)");
  MEMCHK(c, c->h_relo.reserve(stage_bytes), "hipHostMalloc((void **)&c->h_relo, stage_bytes, hipHostMallocDefault)");
  return LFVIO_OK;
}

// the route itself: the window and the relo table are valid (relo_check)
int relo_route(lfvio_ctx *c, const LfvioWindow *in, const LfvioRelo *relo, LfvioSolution *out, double *relo_pose_out) {
  const int N = in->num_landmarks, M = in->num_observations, K = relo->num_matches;
  if (N > RELO_MAX_LM) {
    c->err = "lfvio_solve_relo: more than " + std::to_string(RELO_MAX_LM) + " landmarks";
    return LFVIO_ERR_ARG;
  }
  const LfvioPrior *pr = (in->prior && in->prior->valid) ? in->prior : nullptr;
  const int pn = pr ? pr->n : 0;
  const int row_relo = 2 * (M - N), row_imu = row_relo + 2 * K, row_prior = row_imu + 15 * LFVIO_WINDOW_SIZE, R = row_prior + pn;
  const ReloLayout L = relo_layout(N, M, K, R, pn);
  if (int rc = relo_grow(c, L.total, L.in_end)) return rc;
  char *h = c->h_relo, *d = c->d_relo;
  // header
  ReloDev *H = (ReloDev *)h;
  std::memset((void *)H, 0, sizeof(ReloDev));
  H->N = N, H->M = M, H->K = K, H->R = R, H->max_iter = in->max_num_iterations;
  H->est_ex = in->estimate_extrinsic != 0, H->est_td = in->estimate_td != 0, H->relo_on = K > 0;
  H->prior_n = pn, H->prior_nb = pr ? pr->num_blocks : 0;
  H->row_relo = row_relo, H->row_imu = row_imu, H->row_prior = row_prior;
  H->sqrt_info = in->sqrt_info, H->tr_ro = in->tr, H->row = in->row;
  for (int k = 0; k < 3; k++) H->g[k] = in->g[k];
  auto dp = [&](size_t o) { return (void *)(d + o); };
  H->start = (const int *)dp(L.start), H->off = (const int *)dp(L.off), H->rk = (const int *)dp(L.rk);
  H->pt = (const double *)dp(L.pt), H->vel = (const double *)dp(L.vel), H->ctd = (const double *)dp(L.ctd), H->uvy = (const double *)dp(L.uvy);
  H->mp = (const double *)dp(L.mp), H->lam0 = (const double *)dp(L.lam0);
  for (int f = 0; f < LFVIO_WINDOW_SIZE; f++) H->imu[f] = in->imu[f];
  if (pr) {
    for (int b = 0; b < pr->num_blocks; b++) {
      H->prior_kind[b] = pr->blocks[b].kind, H->prior_frame[b] = pr->blocks[b].frame, H->prior_idx[b] = pr->block_idx[b];
      for (int k = 0; k < 9; k++) H->prior_x0[b][k] = pr->block_x0[b][k];
    }
  }
  H->prior_J = (const double *)dp(L.pJ), H->prior_r = (const double *)dp(L.pr);
  std::memcpy(H->x0.f.pose, in->para_pose, sizeof H->x0.f.pose);
  std::memcpy(H->x0.f.sb, in->para_speed_bias, sizeof H->x0.f.sb);
  std::memcpy(H->x0.f.ex, in->para_ex_pose, sizeof H->x0.f.ex);
  H->x0.f.td = in->para_td;
  std::memcpy(H->x0.relo, relo->relo_pose, sizeof H->x0.relo);
  H->lam[0] = (double *)dp(L.lam0w), H->lam[1] = (double *)dp(L.lam1w);
  H->J = (double *)dp(L.J), H->gpart = (double *)dp(L.gpart), H->Hs = (double *)dp(L.Hs), H->Sg = (double *)dp(L.Sg), H->gs = (double *)dp(L.gs), H->W = (double *)dp(L.W);
  H->h = (double *)dp(L.h), H->gl = (double *)dp(L.gl), H->lcost = (double *)dp(L.lcost);
  H->scale_l = (double *)dp(L.scale_l), H->diag_l = (double *)dp(L.diag_l), H->gn_l = (double *)dp(L.gn_l), H->stp_l = (double *)dp(L.stp_l);
  H->hs = (double *)dp(L.hs), H->gsl = (double *)dp(L.gsl);
  for (int i = 0; i < RK; i++) {
    const bool ex = i >= off_ex() && i < off_ex() + 6, td = i == off_td(), rl = i >= RO;
    H->act[i] = !((ex && !H->est_ex) || (td && !H->est_td) || (rl && !H->relo_on));
  }
  // inputs
  if (N > 0) {
    std::memcpy(h + L.start, in->start_frame, (size_t)N * 4);
    std::memcpy(h + L.off, in->obs_offset, (size_t)(N + 1) * 4);
    std::memcpy(h + L.pt, in->obs_point, (size_t)M * 24);
    std::memcpy(h + L.vel, in->obs_velocity, (size_t)M * 24);
    std::memcpy(h + L.ctd, in->obs_cur_td, (size_t)M * 8);
    std::memcpy(h + L.uvy, in->obs_uv_y, (size_t)M * 8);
    std::memcpy(h + L.lam0, in->inv_depth, (size_t)N * 8);
  }
  int *rk = (int *)(h + L.rk);
  for (int l = 0; l < N; l++) rk[l] = -1;
  for (int k = 0; k < K; k++) rk[relo->landmark[k]] = k;
  if (K > 0) std::memcpy(h + L.mp, relo->match_point, (size_t)K * 16);
  if (pr) {
    std::memcpy(h + L.pJ, pr->linearized_jacobians, (size_t)pn * pn * 8);
    std::memcpy(h + L.pr, pr->linearized_residuals, (size_t)pn * 8);
  }
  ReloDev *Dd = (ReloDev *)d;
  HIPCHK(c, hipMemcpyAsync(d, h, L.in_end, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_relo_setup, dim3(1), dim3(64), 0, c->stream, Dd, c->init_radius, c->fn_tol);
  HIPCHK(c, hipGetLastError());
  const int lm_wgs = (N + RELO_LM_WG - 1) / RELO_LM_WG;
  const bool capped = in->max_solver_time_in_seconds > 0.0;
  const auto t_start = std::chrono::steady_clock::now();
  int done = 0, passes = 0;
  const int max_passes = std::max(in->max_num_iterations, 0) + 8;
  while (!done) {
    hipLaunchKernelGGL(k_relo_eval<true>, dim3(lm_wgs + LFVIO_WINDOW_SIZE + 1), dim3(64), 0, c->stream, Dd);
    hipLaunchKernelGGL(k_relo_gram, dim3(RELO_GTILES, RELO_GCH), dim3(256), 0, c->stream, Dd);
    hipLaunchKernelGGL(k_relo_solve, dim3(1), dim3(RELO_SOLVE_THREADS), RELO_SOLVE_LDS, c->stream, Dd, 0);
    hipLaunchKernelGGL(k_relo_schur, dim3(RELO_STILES), dim3(256), 0, c->stream, Dd);
    hipLaunchKernelGGL(k_relo_solve, dim3(1), dim3(RELO_SOLVE_THREADS), RELO_SOLVE_LDS, c->stream, Dd, 1);
    hipLaunchKernelGGL(k_relo_eval<false>, dim3(lm_wgs + LFVIO_WINDOW_SIZE + 1), dim3(64), 0, c->stream, Dd);
    hipLaunchKernelGGL(k_relo_decide, dim3(1), dim3(64), 0, c->stream, Dd);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&c->relo_done_word, &Dd->tr.done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    done = c->relo_done_word;
    passes++;
    if (!done && (passes >= max_passes ||
                  (capped && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= in->max_solver_time_in_seconds))) {
      hipLaunchKernelGGL(k_relo_stop, dim3(1), dim3(64), 0, c->stream, Dd);
      HIPCHK(c, hipGetLastError());
      break;
    }
  }
  c->last_passes = passes;
  // download: the loop header, then the state it points at
  std::vector<char> hd(sizeof(ReloDev));
  HIPCHK(c, hipMemcpyAsync(hd.data(), d, sizeof(ReloDev), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const ReloDev *R0 = (const ReloDev *)hd.data();
  const TRState *T = &R0->tr;
  const int cur = T->cur & 1;
  std::vector<double> lam((size_t)std::max(N, 1));
  if (N > 0) {
    HIPCHK(c, hipMemcpyAsync(lam.data(), d + (cur ? L.lam1w : L.lam0w), (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  const ReloX &x = R0->x[cur];
  if (int rc = check_solution(c, T, (const double *)&x, sizeof(ReloX) / 8, lam.data(), N)) return relo_refused(c, rc);
  unpack_solution(T, x.f, lam.data(), N, nullptr, out);
  std::memcpy(relo_pose_out, x.relo, sizeof x.relo);
  return LFVIO_OK;
}

}  // namespace

int lfvio_solve_relo(lfvio_ctx *c, const LfvioWindow *in, const LfvioRelo *relo, LfvioSolution *out, double relo_pose_out[LFVIO_SIZE_POSE]) {
  if (!c || !in || !relo || !out || !relo_pose_out) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = relo_check(c, in, relo)) return rc;
  if (relo->num_matches == 0 && !c->relo_force) {
    // no relo factor: Ceres drops the unused relo_Pose block, the solve is the plain one (estimator.cpp:777-808)
    const int rc = lfvio_solve(c, in, out);
    if (rc == LFVIO_OK) std::memcpy(relo_pose_out, relo->relo_pose, sizeof(double) * LFVIO_SIZE_POSE);
    return rc;
  }
  if (int rc = join_inflight(c)) return rc;
  return relo_route(c, in, relo, out, relo_pose_out);
}
