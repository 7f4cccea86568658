// debug.inc — the parity / inspection hooks of include/lfvio_debug.h (lfvio_debug_group_inject_failure apart: group.inc).  Included by
// lfvio_hip.hip inside its extern "C" block.  Host code only: the hooks launch what the product launches, through the product's own
// launch functions, and copy down what that left.
//
// A hook that runs a pass and reads a slot is built from three pieces: debug_pass_launch (checks, k_setup, header pokes, sweep and
// solve of a Route), a SlotReader over the slot, and expand_W for the landmark rows; debug_pass_copy is those two readers over
// everything of LfvioPassIO.

namespace {

bool slots_ok(const lfvio_ctx *c, int count) { return c && c->d_base && count > 0 && count <= c->batch; }

// Memory of one slot, read down synchronously.  A NULL destination or zero bytes is success without a copy.
struct SlotReader {
  const char *d;
  SlotReader(lfvio_ctx *c, int slot) : d(c->d_base + (size_t)slot * c->L.total) {}
  hipError_t operator()(void *dst, size_t off, size_t bytes) const { return !dst || !bytes ? hipSuccess : hipMemcpy(dst, d + off, bytes, hipMemcpyDeviceToHost); }
};

// One field of the trust-region header (offset within TRState) of slots [0, count), written synchronously.
int poke_header(lfvio_ctx *c, int count, size_t field_offset, const void *value, size_t bytes) {
  for (int s = 0; s < count; s++)
    HIPCHK(c, hipMemcpy(c->d_base + (size_t)s * c->L.total + offsetof(Slot, tr) + field_offset, value, bytes, hipMemcpyHostToDevice));
  return LFVIO_OK;
}

// W [N][KC] in device landmark order, from the rows the route's sweep left: the compact rows behind the roles, the transposed ones
// behind k_linw / k_linb.  A landmark's span: its track's frames, then ex (6) and td.
int expand_W(lfvio_ctx *c, const Route &r, const SlotReader &get, int N, double *W) {
  const Layout &L = c->L;
  std::vector<int> woff(N + 1), lst(N), lcn(N);
  HIPCHK(c, get(woff.data(), L.lm_woff, sizeof(int) * (N + 1)));
  HIPCHK(c, get(lst.data(), L.lm_start, sizeof(int) * N));
  HIPCHK(c, get(lcn.data(), L.lm_cnt, sizeof(int) * N));
  const bool compact = r.sweep == Route::ROLES;
  // (the transposed rows: column pair p of landmark l at [p][l], the pairs wld landmarks apart)
  const size_t wld = r.sweep == Route::LINB ? (size_t)L.capLmBlocks * LM_BLOCK : (size_t)SPEC_MAX_LM;
  if (compact ? (woff[N] < 0 || (size_t)woff[N] > (size_t)N * (KC + 2)) : (size_t)N > wld) return LFVIO_ERR_ARG;
  std::vector<double> rows(compact ? (size_t)woff[N] + 1 : (size_t)WT_PAIRS * wld * 2);
  HIPCHK(c, get(rows.data(), compact ? L.W : L.Wt, compact ? sizeof(double) * woff[N] : rows.size() * 8));
  std::fill(W, W + (size_t)N * KC, 0.0);
  for (int dl = 0; dl < N; dl++)
    for (int ci = 0; ci < 6 * lcn[dl] + 7; ci++) {
      const int col = ci < 6 * lcn[dl] ? 6 * lst[dl] + ci : 66 + (ci - 6 * lcn[dl]);
      W[(size_t)dl * KC + col] = compact ? rows[(size_t)woff[dl] + ci] : rows[((size_t)(col >> 1) * wld + dl) * 2 + (col & 1)];
    }
  return LFVIO_OK;
}

// The first half of a pass over the resident slots [0, count), by the route given: k_setup, the header's mu and radius where the caller
// gives one (> 0), the sweep and the dense solve.  Enqueued, not waited for.  The one place that checks the arguments, that every slot
// is resident, and joins the call in flight.
int debug_pass_launch(lfvio_ctx *c, const Route &r, int count, int slot, double mu, double radius) {
  if (!slots_ok(c, count) || slot < 0 || slot >= count) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = join_inflight(c)) return rc;
  for (int s = 0; s < count; s++)
    if (!c->info[s].resident) return LFVIO_ERR_ARG;
  launch_setup(c, r, MODE_SOLVE);
  if (mu > 0.0) {  // (k_setup arms the header with Ceres' initial mu: the caller's replaces it before the sweep weighs the landmarks with it)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = poke_header(c, count, offsetof(TRState, mu), &mu, sizeof mu)) return rc;
  }
  if (radius > 0.0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = poke_header(c, count, offsetof(TRState, radius), &radius, sizeof radius)) return rc;
  }
  launch_sweep(c, r, MODE_SOLVE, true);
  launch_solve(c, count, r.sweep == Route::LINW);
  HIPCHK(c, hipGetLastError());  // (a launch that was refused — resources, LDS — must not pass as a result left by an earlier one)
  return LFVIO_OK;
}

// What that half left in slot `slot` (the stream has been waited for): plain copies.  Returns the sweep kernel, < 0 on error.
int debug_pass_copy(lfvio_ctx *c, const Route &r, int slot, LfvioPassIO *io) {
  const Layout &L = c->L;
  const int N = c->info[slot].N;
  const SlotReader get(c, slot);
  int hdr[2] = {0, 0}, prior[2] = {0, 0};  // est_ex, est_td | prior_valid, prior_n
  HIPCHK(c, get(hdr, offsetof(Slot, est_ex), sizeof hdr));
  HIPCHK(c, get(prior, offsetof(Slot, prior_valid), sizeof prior));
  static_assert(offsetof(Slot, est_td) == offsetof(Slot, est_ex) + sizeof(int) && offsetof(Slot, prior_n) == offsetof(Slot, prior_valid) + sizeof(int), "read in pairs");
  io->est_ex = hdr[0], io->est_td = hdr[1], io->prior_n = prior[0] ? prior[1] : 0, io->num_landmarks = N;
  if (io->prior_n < 0 || io->prior_n > KP) return LFVIO_ERR_ARG;
  HIPCHK(c, get(io->H, L.xch + (size_t)XOFF_H * 8, (size_t)PACKED * 8));
  HIPCHK(c, get(io->gp, L.xch + (size_t)XOFF_G * 8, KP * 8));
  HIPCHK(c, get(io->schur, L.xch + (size_t)XOFF_S * 8, SCHUR_LEN * 8));
  HIPCHK(c, get(io->lm_sum, offsetof(Slot, lm_sum), LMS * 8));
  HIPCHK(c, get(io->imu_out, L.imu_out, (size_t)LFVIO_WINDOW_SIZE * IMU_OUT * 8));
  HIPCHK(c, get(io->prior_A, L.prior_A, (size_t)io->prior_n * io->prior_n * 8));
  HIPCHK(c, get(io->prior_cmap, offsetof(Slot, prior_cmap), KP * sizeof(int)));
  HIPCHK(c, get(&io->prior_cost, offsetof(Slot, prior_g) + (size_t)KP * 8, 8));
  HIPCHK(c, get(io->a, L.a, (size_t)N * 8));
  HIPCHK(c, get(io->b, L.b, (size_t)N * 8));
  if (io->W && N)
    if (int rc = expand_W(c, r, get, N, io->W)) return rc;
  HIPCHK(c, get(io->scale_p, offsetof(Slot, scale_p), KP * 8));
  HIPCHK(c, get(io->diag_p, offsetof(Slot, diag_p), KP * 8));
  HIPCHK(c, get(io->grad_p, offsetof(Slot, grad_p), KP * 8));
  HIPCHK(c, get(io->gn_p, offsetof(Slot, gn_p), KP * 8));
  HIPCHK(c, get(io->uc_grad, offsetof(Slot, uc_grad), WLD * 8));
  HIPCHK(c, get(io->uc_gn, offsetof(Slot, uc_gn), WLD * 8));
  TRHead th;
  HIPCHK(c, get(&th, offsetof(Slot, tr), sizeof th));
  if (io->q) std::copy(th.q, th.q + Q_COUNT, io->q);
  io->alpha = th.alpha, io->grad_sq_total = th.grad_sq_total, io->x_cost = th.x_cost, io->mu = th.mu, io->chol_fail = th.chol_fail;
  return r.sweep;
}

void step_header_from(LfvioStepHeader &h, const TRHead &t, int max_iter) {
  h.radius = t.radius, h.mu = t.mu, h.x_cost = t.x_cost, h.x_norm = t.x_norm, h.cand_cost = t.cand_cost, h.model_cost_change = t.model_cost_change;
  h.alpha = t.alpha, h.grad_sq_total = t.grad_sq_total, h.gn_sq_total = t.gn_sq_total, h.grad_gn_total = t.grad_gn_total, h.gmax_pose = t.gmax_pose;
  h.function_tolerance = t.function_tolerance;
  std::copy(t.q, t.q + Q_COUNT, h.q);
  h.iteration = t.iteration, h.cur = t.cur, h.do_lin = t.do_lin, h.do_schur = t.do_schur, h.done = t.done, h.termination = t.termination;
  h.chol_fail = t.chol_fail, h.num_succ = t.num_succ, h.num_unsucc = t.num_unsucc, h.consec_invalid = t.consec_invalid, h.trace_len = t.trace_len;
  h.skip_step = t.skip_step, h.spec_n = t.spec_n, h.max_iter = max_iter;
}

// Which kernel linearizes a launch over the resident slots [0, count): 0 k_lin (+ k_sum), 1 k_linw, 2 k_linb (+ k_sumb).
int sweep_kernel_of(lfvio_ctx *c, int count) { return !slots_ok(c, count) ? LFVIO_ERR_ARG : route_for(c, count, MODE_SOLVE).sweep; }

}  // namespace

// That pass on a freshly uploaded window, the role sweep whatever the route (without the Wt clear of k_linw's k_setup): the packed H_pp
// read is k_sum's.  Its own: H unpacked to the full square, the landmarks in the caller's order.
int lfvio_debug_linearize(lfvio_ctx *c, const LfvioWindow *in, double *Hpp, double *gp, double *a, double *b, double *W,
                          double *cost) {
  if (!c || !in) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  int rc = reserve(c, 1, in->num_landmarks, in->num_observations);
  if (rc) return rc;
  if ((rc = upload_window(c, 0, in))) return rc;
  Route r = route_for(c, 1, MODE_SOLVE);
  r.sweep = Route::ROLES, r.setup.bits = 0;
  if ((rc = debug_pass_launch(c, r, 1, 0, 0.0, 0.0))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int N = in->num_landmarks;
  std::vector<double> packed(PACKED), av(N), bv(N), Wv((size_t)N * KC);
  LfvioPassIO io{};
  io.H = packed.data(), io.gp = gp, io.a = av.data(), io.b = bv.data(), io.W = Wv.data();
  if ((rc = debug_pass_copy(c, r, 0, &io)) < 0) return rc;
  for (int i = 0; i < KP; i++)
    for (int j = 0; j < KP; j++) Hpp[i * KP + j] = packed[pidx(i, j)];
  const std::vector<int> &perm = c->info[0].perm;
  for (int dl = 0; dl < N; dl++) {
    a[perm[dl]] = av[dl], b[perm[dl]] = bv[dl];
    std::copy(Wv.begin() + (size_t)dl * KC, Wv.begin() + (size_t)(dl + 1) * KC, W + (size_t)perm[dl] * KC);
  }
  *cost = io.x_cost;
  return LFVIO_OK;
}

// The mu-retry path (do_schur without do_lin: k_lin's landmark blocks redo only the Schur SYRK from the stored W rows)
// against a full linearization at the same mu.  Returns the largest absolute difference of the Schur sums (expected 0).
int lfvio_debug_schur_repeat(lfvio_ctx *c, const LfvioWindow *in, double mu, double *max_abs_diff) {
  if (!c || !in || !max_abs_diff) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  int rc = reserve(c, 1, in->num_landmarks, in->num_observations);
  if (rc) return rc;
  if ((rc = upload_window(c, 0, in))) return rc;
  const Route r = route_for(c, 1, MODE_SOLVE);  // (lfvio_debug_configure "linw" 2: the window-resident sweep, for one window)
  const SlotReader get(c, 0);
  auto run = [&](int do_lin, std::vector<double> &out) -> int {
    const int do_schur = 1;
    if (int e = poke_header(c, 1, offsetof(TRState, mu), &mu, sizeof mu)) return e;
    if (int e = poke_header(c, 1, offsetof(TRState, do_lin), &do_lin, sizeof do_lin)) return e;
    if (int e = poke_header(c, 1, offsetof(TRState, do_schur), &do_schur, sizeof do_schur)) return e;
    launch_sweep(c, r, MODE_SOLVE, true);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out.resize(SCHUR_LEN);
    HIPCHK(c, get(out.data(), c->L.xch + sizeof(double) * XOFF_S, sizeof(double) * SCHUR_LEN));
    return LFVIO_OK;
  };
  launch_setup(c, r, MODE_SOLVE);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<double> first, repeat, full;
  const double mu1 = mu;
  mu = 1e-8;
  if ((rc = run(1, first))) return rc;   // ordinary first pass (fixes the Jacobi scaling: k_solve does that, so run it)
  launch_solve(c, 1, r.sweep == Route::LINW);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  mu = mu1;
  if ((rc = run(0, repeat))) return rc;  // Schur only, new mu
  if ((rc = run(1, full))) return rc;    // everything again at the new mu
  double m = 0, ref = 0;
  for (int i = 0; i < SCHUR_LEN; i++) m = std::max(m, std::fabs(repeat[i] - full[i])), ref = std::max(ref, std::fabs(full[i] - first[i]));
  *max_abs_diff = m;
  return ref > 0 ? LFVIO_OK : LFVIO_ERR_ARG;  // the new mu must have changed the sums, or the check proves nothing
}

// Post-Schur system A', b' of the last marginalization of slot 0 (n x n, n).
int lfvio_debug_marg_system(lfvio_ctx *c, int n, double *A, double *b) {
  if (!c || !c->d_base) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = join_inflight(c)) return rc;
  if (n < 0 || n > 76) return LFVIO_ERR_ARG;  // (k_marg_solve forms no larger system: see the upload)
  if (n == 0) return LFVIO_OK;
  char *d = c->d_base + c->L.mscr;
  if (c->shadow) {
    // A prior that a worker delivered (kernels_spec.h) was formed in the worker's shadow slot, and so were its A', b': slot 0's
    // scratch still holds those of an earlier marginalization.  The shadow slot whose prior is the one in slot 0, bit for bit, is
    // where the system of that prior lies (a worker that lost the call to the loop's own tail holds the same bits or an older state's).
    // The round that formed it worked on the state the call ended with — x[0] of the shadow after k_spec_begin's gauge fix is x[cur] of
    // slot 0 after the loop's, the same function on the same numbers: a shadow that still holds the same prior from an EARLIER call on
    // the same window, and has begun a round on another state since, has other scratch.
    const size_t head = offsetof(LfvioPrior, linearized_jacobians), bytes = head + sizeof(double) * n * n;
    std::vector<char> p0(bytes), pw(bytes);
    HIPCHK(c, hipMemcpy(p0.data(), c->d_base + offsetof(Slot, prior_out), bytes, hipMemcpyDeviceToHost));
    const LfvioPrior *h0 = (const LfvioPrior *)p0.data();
    int cur = 0;
    FrameState x0, xw;
    HIPCHK(c, hipMemcpy(&cur, c->d_base + offsetof(Slot, tr) + offsetof(TRState, cur), sizeof cur, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&x0, c->d_base + offsetof(Slot, x) + sizeof(FrameState) * (cur & 1), sizeof x0, hipMemcpyDeviceToHost));
    for (int wk = 0; wk < lfvio_ctx::WORKERS && h0->valid == 1 && h0->n == n; wk++) {
      char *ds = c->d_base + (size_t)(c->batch + wk) * c->L.total;
      HIPCHK(c, hipMemcpy(pw.data(), ds + offsetof(Slot, prior_out), bytes, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&xw, ds + offsetof(Slot, x), sizeof xw, hipMemcpyDeviceToHost));
      const LfvioPrior *hw = (const LfvioPrior *)pw.data();
      if (std::memcmp(&x0, &xw, sizeof x0) == 0 && hw->valid == 1 && hw->n == n && std::memcmp(p0.data() + head, pw.data() + head, bytes - head) == 0) {
        d = ds + c->L.mscr;
        break;
      }
    }
  }
  HIPCHK(c, hipMemcpy(A, d + sizeof(double) * (92 * 92 + 96), sizeof(double) * n * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(b, d + sizeof(double) * (92 * 92 + 96 + n * n), sizeof(double) * n, hipMemcpyDeviceToHost));
  return LFVIO_OK;
}

int lfvio_debug_read_clocks(lfvio_ctx *c, long long *out32) {
  if (!c || !c->d_base) return LFVIO_ERR_ARG;
  if (int rc = join_inflight(c)) return rc;
  HIPCHK(c, hipMemcpy(out32, c->d_base + offsetof(Slot, dbg), sizeof(long long) * 32, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(out32 + 32, c->d_base + offsetof(Slot, jtrace), sizeof(double) * 32, hipMemcpyDeviceToHost));
  return LFVIO_OK;
}

// Average duration (ms) of `reps` launches of one pipeline kernel on slots [0, count), measured with
// HIP events on the context's own stream.  which: 0 k_lin (with the Schur SYRK of the landmark blocks), 2 k_sum, 3 k_solve.
// The slots must hold an uploaded window; the trust-region flags are re-armed by k_setup first.
int lfvio_debug_time_kernel(lfvio_ctx *c, int which, int count, int reps, double *avg_ms) {
  if (!slots_ok(c, count) || reps <= 0) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = join_inflight(c)) return rc;
  const Route r = route_for(c, count, MODE_SOLVE);
  const Grid &g = r.g;
  const size_t st = c->L.total;
  const bool lw = r.sweep == Route::LINW, lb = r.sweep == Route::LINB;
  const bool offs = (r.offs & 2) != 0;  // the instantiation the passes behind the first one run (with_offs)
  // which kernel the launch would take is settled before anything is created or enqueued
  if ((which == 11 || which == 12) && !lw) {
    c->err = "the resident windows are not linearized by k_linw";
    return LFVIO_ERR_ARG;
  }
  if (which >= 15 && which <= 17 && !lb) {
    c->err = "the resident window is not linearized by k_linb";
    return LFVIO_ERR_ARG;
  }
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0));
  if (hipError_t e = hipEventCreate(&e1); e != hipSuccess) {
    (void)hipEventDestroy(e0);
    HIPCHK(c, e);
  }
  launch_setup(c, r, MODE_SOLVE);
  // one full linearization so that every kernel has valid inputs (the roles but for the k_linb kernels)
  Route full = r;
  if (lb && !(which >= 15 && which <= 17)) full.sweep = Route::ROLES;
  launch_sweep(c, full, MODE_SOLVE, offs);
  if (which == 14) launch_solve(c, count, lw);
  if (which == 17) launch_solve(c, count, false);

  HIPCHK(c, hipEventRecord(e0, c->stream));
  for (int rep = 0; rep < reps; rep++) {
    switch (which) {
      case 0: launch_lin(c, r, MODE_SOLVE, offs); break;
      case 2: launch_sum(c, r, MODE_SOLVE); break;  // k_presum + k_sum for large windows
      case 8: case 9: case 10: case 18: {  // k_lin by role: landmark blocks | Gram chunks | IMU factors + prior | IMU factors alone
        const int gram_wgs = (g.ch + 3) / 4;
        const int gx = which == 8 ? g.lw : which == 9 ? gram_wgs : which == 18 ? LFVIO_WINDOW_SIZE : LFVIO_WINDOW_SIZE + 1;
        hipLaunchKernelGGL((k_lin<LIN_ROLE_ALL, false>), dim3(gx, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st, MODE_SOLVE, which == 8 ? g.lw : 0,
                           which == 9 ? gram_wgs : 0, slot_args(c->L));
      } break;
      case 4: case 5: case 6: case 7: {  // k_setup by role: state + table | + IMU sqrt_info | + prior J0^T J0 | + inverse depths
        const SetupLaunch sl = setup_launch(c, count, g.lm, false);  // (the grid the product launches: compact for a resident batch)
        const int wgs = (sl.bits & 4) ? 3 : SETUP_WGS, gx = which == 4 ? 1 : which == 5 ? 2 : which == 6 ? wgs : sl.gx;
        hipLaunchKernelGGL(k_setup, dim3(gx, count), dim3(256), 0, c->stream, c->d_base, st, MODE_SOLVE, sl.bits);
      } break;
      case 11: case 12: launch_sweep(c, r, MODE_SOLVE, offs); break;  // the window-resident sweep of a batch (k_linw: pose-side factors, visual sweep, Schur)
      case 13: launch_solve(c, count, lw); break;
      case 14: hipLaunchKernelGGL(k_stepw, dim3(1, count), dim3(STEPW_LAUNCH_THREADS), 0, c->stream, c->d_base, st); break;  // (not idempotent: a few reps only)
      // a large single window, group by group: 15 the strip sweep (k_linb), 16 the sum of its partials (k_sumb), 17 the landmark
      // back-substitution from the transposed rows (k_backsub_wt)
      case 15: hipLaunchKernelGGL(k_linb<false>, dim3(r.linb_gx, count), dim3(LW_THREADS), LW_LDS_BYTES, c->stream, c->d_base, st, linw_args(c)); break;
      case 16: hipLaunchKernelGGL(k_sumb, dim3(LINB_SUM_GRID, count), dim3(LINB_SUM_THREADS), 0, c->stream, c->d_base, st, linw_args(c)); break;
      case 17: hipLaunchKernelGGL(k_backsub_wt, dim3(g.lm, count), dim3(64), 0, c->stream, c->d_base, st, c->L.capLmBlocks * LM_BLOCK); break;
      default: launch_solve(c, count); break;
    }
  }
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  *avg_ms = (double)ms / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return LFVIO_OK;
}

// One linearization + dense solve of the resident slots [0, count) from their uploaded state — k_setup, the sweep and the solve of the
// launch's own route (lfvio_debug_configure "linw"), at the caller's mu where it gives one — and everything k_solve_dense read and wrote in
// slot `slot` (include/lfvio_debug.h).  tests/test_solve_hp.py holds the solve to a 50-digit reference formed from these very inputs.
int lfvio_debug_pass_io(lfvio_ctx *c, int count, int slot, double mu, LfvioPassIO *io) {
  if (!slots_ok(c, count) || !io) return LFVIO_ERR_ARG;
  const Route r = route_for(c, count, MODE_SOLVE);
  if (int rc = debug_pass_launch(c, r, count, slot, mu, 0.0)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return debug_pass_copy(c, r, slot, io);
}

// The whole pass: the half above, then the step half through launch_step_half — the function the loop's passes go through — and what it
// read and wrote in slot `slot` (include/lfvio_debug.h).  tests/test_step_hp.py holds every stage to a 50-digit reference formed from these
// very inputs.
int lfvio_debug_step_io(lfvio_ctx *c, int count, int slot, double mu, double radius, int spec, LfvioStepIO *io) {
  if (!slots_ok(c, count) || !io) return LFVIO_ERR_ARG;
  const Route r = route_for(c, count, MODE_SOLVE);
  // (more than one candidate only where the loop itself always speculates: one window whose back-substitution rides in the dogleg)
  const bool speculates = count == 1 && r.g.lm <= DOGLEG_INLINE_BLOCKS;
  if (spec < 1 || spec > 1 + SPEC_EXTRA || (spec > 1 && !speculates)) return LFVIO_ERR_ARG;
  static_assert(sizeof(FrameState) == LFVIO_STATE_DOUBLES * sizeof(double), "LFVIO_STATE_DOUBLES is a FrameState");
  if (int rc = debug_pass_launch(c, r, count, slot, mu, radius)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = debug_pass_copy(c, r, slot, &io->pass); rc < 0) return rc;
  const Layout &L = c->L;
  const int N = c->info[slot].N;
  const SlotReader get(c, slot);
  int nblk = 0, max_iter = 0;
  HIPCHK(c, get(&nblk, offsetof(Slot, nLmBlocks), sizeof nblk));
  HIPCHK(c, get(&max_iter, offsetof(Slot, max_iter), sizeof max_iter));
  if (nblk < 0 || nblk > L.capLmBlocks) return LFVIO_ERR_ARG;
  io->num_blocks = nblk, io->tab_bytes = (int)sizeof(Tab), io->spec = spec, io->head_valid = 0, io->stepw = 0;
  TRHead th;
  HIPCHK(c, get(&th, offsetof(Slot, tr), sizeof th));
  const int cur = th.cur & 1;
  step_header_from(io->head, th, max_iter);
  // read by the step half (the solve is behind us, nothing of this is written by the step half)
  HIPCHK(c, get(io->scale_l, L.scale_l, (size_t)N * 8));
  HIPCHK(c, get(io->diag_l, L.diag_l, (size_t)N * 8));
  HIPCHK(c, get(io->grad_l, L.grad_l, (size_t)N * 8));
  HIPCHK(c, get(io->einv_l, L.einv_l, (size_t)N * 8));
  HIPCHK(c, get(io->lam, L.lam[cur], (size_t)N * 8));
  HIPCHK(c, get(io->x, offsetof(Slot, x) + (size_t)cur * sizeof(FrameState), sizeof(FrameState)));
  // what the bookkeeping reads: copied in front of it, where it is a kernel of its own (an accepted speculative candidate is copied
  // over candidate 0 by it), behind k_stepw otherwise (one candidate, which its bookkeeping leaves where it is)
  int crc = LFVIO_OK;
  auto copy_candidates = [&]() -> int {
    TRHead t;
    HIPCHK(c, get(&t, offsetof(Slot, tr), sizeof t));
    if (io->head_valid) step_header_from(io->head, t, max_iter);
    else io->head.gn_sq_total = t.gn_sq_total, io->head.grad_gn_total = t.grad_gn_total, io->head.gmax_pose = t.gmax_pose, io->head.spec_n = t.spec_n;
    HIPCHK(c, get(io->gn_l, L.gn_l, (size_t)N * 8));
    HIPCHK(c, get(io->d1, L.d1, (size_t)N * 8));
    HIPCHK(c, get(io->d2, L.d2, (size_t)N * 8));
    HIPCHK(c, get(io->step_p, offsetof(Slot, step_p), KP * 8));
    std::vector<double> part;
    for (int z = 0; z < spec; z++) {
      if (io->coef) {
        double *o = io->coef + 5 * z;
        o[0] = z ? t.cgE[z - 1] : t.cg, o[1] = z ? t.cnE[z - 1] : t.cn, o[2] = z ? t.snE[z - 1] : t.dogleg_step_norm;
        o[3] = z ? t.step_sqE[z - 1] : t.step_sq_pose, o[4] = z ? t.xn2E[z - 1] : t.xn2_pose_cand;
      }
      const size_t xo = z ? offsetof(Slot, xE) + (size_t)(z - 1) * sizeof(FrameState) : offsetof(Slot, x) + (size_t)(cur ^ 1) * sizeof(FrameState);
      const size_t to = z ? offsetof(Slot, tabE) + (size_t)(z - 1) * sizeof(Tab) : offsetof(Slot, tab) + (size_t)(cur ^ 1) * sizeof(Tab);
      HIPCHK(c, get(io->cand_x ? io->cand_x + (size_t)z * LFVIO_STATE_DOUBLES : nullptr, xo, sizeof(FrameState)));
      HIPCHK(c, get(io->cand_tab ? io->cand_tab + (size_t)z * sizeof(Tab) : nullptr, to, sizeof(Tab)));
      HIPCHK(c, get(io->cand_lam ? io->cand_lam + (size_t)z * N : nullptr, z ? L.lamE[z - 1] : L.lam[cur ^ 1], (size_t)N * 8));
      HIPCHK(c, get(io->pose_cost ? io->pose_cost + 11 * z : nullptr, z ? offsetof(Slot, pose_costE) + (size_t)(z - 1) * 16 * 8 : offsetof(Slot, pose_cost), 11 * 8));
      if (io->block_sums && nblk) {
        // (candidates 1 .. hold the blocks of windows of at most SPEC_MAX_LM landmarks: the only ones that speculate)
        if (z && nblk > SPEC_MAX_LM / 64) return LFVIO_ERR_ARG;
        part.resize((size_t)nblk * LMS);
        HIPCHK(c, get(part.data(), z ? L.cost_partE + (size_t)(z - 1) * (SPEC_MAX_LM / 64) * LMS * 8 : L.cost_part, part.size() * 8));
        for (int b = 0; b < nblk; b++) std::copy(part.begin() + (size_t)b * LMS, part.begin() + (size_t)b * LMS + 5, io->block_sums + ((size_t)z * nblk + b) * 5);
      }
    }
    return LFVIO_OK;
  };
  Pass ps;
  ps.speculate = spec > 1;  // (first and last: the bookkeeping is k_decide, the form behind the last pass of a sequence)
  launch_step_half(c, r, ps, pass_merges(r), spec, [&] {
    io->head_valid = 1;
    const hipError_t e = hipStreamSynchronize(c->stream);
    crc = e != hipSuccess ? LFVIO_ERR_DEVICE : copy_candidates();
  });
  if (crc) return crc;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!io->head_valid) {
    io->stepw = 1;
    if (int rc = copy_candidates()) return rc;
  }
  HIPCHK(c, get(&th, offsetof(Slot, tr), sizeof th));
  step_header_from(io->after, th, max_iter);
  const int ncur = th.cur & 1;
  HIPCHK(c, get(io->trace, offsetof(Slot, tr) + offsetof(TRState, trace), sizeof(LfvioIterationSummary) * LFVIO_MAX_TRACE));
  HIPCHK(c, get(io->x_after, offsetof(Slot, x) + (size_t)ncur * sizeof(FrameState), sizeof(FrameState)));
  HIPCHK(c, get(io->lam_after, L.lam[ncur], (size_t)N * 8));
  HIPCHK(c, get(io->tab_after, offsetof(Slot, tab) + (size_t)ncur * sizeof(Tab), sizeof(Tab)));
  return r.sweep;
}
// Every switch of the debug interface in one call (include/lfvio_debug.h).  The product entry points read no environment: a tool
// that wants LFVIO_DEBUG="key=value,key=value" honoured asks for it with the key "env".
int lfvio_debug_configure(lfvio_ctx *c, const char *key, double value) {
  if (!c || !key) return LFVIO_ERR_ARG;
  const std::string k = key;
  const int iv = (int)value;
  if (k == "env") {
    const char *e = getenv("LFVIO_DEBUG");
    if (!e) return LFVIO_OK;
    std::string all = e;
    for (size_t p = 0; p < all.size();) {
      const size_t q = std::min(all.find(',', p), all.size()), eq = all.find('=', p);
      if (eq != std::string::npos && eq < q) {
        const int rc = lfvio_debug_configure(c, all.substr(p, eq - p).c_str(), atof(all.substr(eq + 1, q - eq - 1).c_str()));
        if (rc) return rc;
      }
      p = q + 1;
    }
    return LFVIO_OK;
  }
  // (switches that change what the captured graphs hold or what an upload builds: the call in flight is joined, the graphs go)
  const bool structural = k == "graph" || k == "linw" || k == "force_eig";
  if (structural) {
    if (int rc = join_inflight(c)) return rc;
  }
  if (k == "graph") c->use_graph = iv != 0;
  else if (k == "first_passes") {
    if (iv < 0) return LFVIO_ERR_ARG;
    c->fixed_passes = iv;
  } else if (k == "spec_count") c->fixed_spec = iv > 0, c->spec_count = iv > 0 ? std::max(1, std::min(1 + SPEC_EXTRA, iv)) : 3;
  else if (k == "function_tolerance") {
    if (!(value >= 0.0)) return LFVIO_ERR_ARG;
    c->fn_tol = value;
  } else if (k == "initial_radius") c->init_radius = value > 0.0 ? value : 1e4;
  else if (k == "linw") {
    if (iv < 0 || iv > 2) return LFVIO_ERR_ARG;
    c->linw_mode = iv;  // (takes effect with the next upload: the plan and its arrays are built there)
  } else if (k == "lm_half") c->lm_half = iv != 0;  // (with the next upload)
  else if (k == "force_eig") c->force_eig = iv != 0;  // (a kernel argument of the captured launches)
  else if (k == "marg_ahead") c->marg_ahead = iv != 0;  // (a flag of the upload: Slot::spec_on)
  else if (k == "break_next_chain") c->debug_break_chain = iv != 0;
  else if (k == "relo_route") c->relo_force = iv != 0;
  else {
    c->err = "lfvio_debug_configure: unknown key '" + k + "'";
    return LFVIO_ERR_ARG;
  }
  if (structural) destroy_graph(c);
  return LFVIO_OK;
}

int lfvio_debug_query(lfvio_ctx *c, const char *key, double *out, int n) {
  if (!c || !key || !out || n <= 0) return LFVIO_ERR_ARG;
  const std::string k = key;
  auto put = [&](std::initializer_list<double> v) {
    int i = 0;
    for (double x : v)
      if (i < n) out[i++] = x;
    return LFVIO_OK;
  };
  if (k == "last_call") return put({(double)c->last_passes, (double)c->last_iters, (double)c->stat_chunks, (double)c->spec_count});
  if (k == "marg_ahead") return put({(double)c->stat_ahead_calls, (double)c->stat_ahead_hits});
  if (k == "upload_times") return put({c->up_us[0], c->up_us[1], c->up_us[2], c->up_us[3]});
  if (k == "sweep_kernel") {  // out[0] in: the number of resident slots the launch would cover
    const int count = (int)out[0], r = sweep_kernel_of(c, count);
    if (r < 0) return r;
    return put({(double)r, route_for(c, count, MODE_SOLVE).split ? 1.0 : 0.0});
  }
  c->err = "lfvio_debug_query: unknown key '" + k + "'";
  return LFVIO_ERR_ARG;
}
