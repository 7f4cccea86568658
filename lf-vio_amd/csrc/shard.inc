// shard.inc — landmark-sharded multi-GPU entry points (SURVEY.md §8e; included inside extern "C").
//
// Each landmark's residuals, Jacobians, H_ll, b_l, W_l and Schur contribution depend only on pose-side
// blocks, never on another landmark (estimator.cpp:755,768), so rank r linearizes landmarks
// [lm_begin, lm_end) only; IMU factors and the prior are added by ONE rank.  Per trust-region iteration:
//   A  linearize local landmarks -> [H_pp | g_p | Schur sums | 5 scalars]   --- sum-all-reduce (151 KB) ---
//   B  every rank solves the identical reduced system, back-substitutes its landmarks -> 2 scalars --- all-reduce ---
//   C  dogleg step, candidate, local candidate cost + model terms -> 5 scalars                   --- all-reduce ---
//   D  identical accept/reject decision on every rank (no broadcast needed)
// The collective itself is the caller's (RCCL via torch.distributed, or raw rccl): the library only
// exposes the device exchange buffer, so it has no MPI/RCCL link dependency.

int lfvio_shard_exchange_len(void) { return XCH_LEN; }
int lfvio_shard_scalar_offset(void) { return XOFF_C; }

double *lfvio_shard_exchange_ptr(lfvio_ctx *c) {
  if (!c || !c->d_base) return nullptr;
  return (double *)(c->d_base + c->L.xch);
}

// the dense solve and the back-substitution of the rank's landmarks (from the transposed rows behind k_linb: route_for)
static void shard_solve(lfvio_ctx *c, const Route &r) {
  launch_solve(c, 1);
  if (r.sweep == Route::LINB) hipLaunchKernelGGL(k_backsub_wt, dim3(r.g.lm, 1), dim3(64), 0, c->stream, c->d_base, c->L.total, c->L.capLmBlocks * LM_BLOCK);
  else hipLaunchKernelGGL(k_backsub, dim3(r.g.lm, 1), dim3(64), 0, c->stream, c->d_base, c->L.total);
}
// the dogleg step and the cost of its candidate on the rank's landmarks
static void shard_candidate(lfvio_ctx *c, const Grid &g) {
  const size_t st = c->L.total;
  const int nb = g.lm + LFVIO_WINDOW_SIZE + 1;
  hipLaunchKernelGGL(k_dogleg<false>, dim3(1, 1), dim3(128), 0, c->stream, c->d_base, st, 1);
  if (nb <= 2048) hipLaunchKernelGGL(k_cost<4>, dim3(nb, 1), dim3(256), 0, c->stream, c->d_base, st, g.lm, 1);
  else hipLaunchKernelGGL(k_cost<1>, dim3(nb, 1), dim3(64), 0, c->stream, c->d_base, st, g.lm, 1);
}

int lfvio_shard_begin(lfvio_ctx *c, const LfvioWindow *in, int lm_begin, int lm_end, int add_pose_side) {
  if (!c || !in || lm_begin < 0 || lm_end < lm_begin || lm_end > in->num_landmarks) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  LfvioWindow sub = *in;
  const int n = lm_end - lm_begin;
  const int o0 = n > 0 ? in->obs_offset[lm_begin] : 0;
  const int o1 = n > 0 ? in->obs_offset[lm_end] : 0;
  c->sh_off.resize(n + 1);
  for (int l = 0; l <= n; l++) c->sh_off[l] = (n > 0 ? in->obs_offset[lm_begin + l] : 0) - o0;
  sub.num_landmarks = n;
  sub.num_observations = o1 - o0;
  sub.start_frame = in->start_frame + lm_begin;
  sub.obs_offset = c->sh_off.data();
  sub.inv_depth = in->inv_depth + lm_begin;
  sub.obs_point = in->obs_point + 3 * (size_t)o0;
  sub.obs_velocity = in->obs_velocity + 3 * (size_t)o0;
  sub.obs_cur_td = in->obs_cur_td + o0;
  sub.obs_uv_y = in->obs_uv_y + o0;
  c->shard_group = (add_pose_side & 4) != 0;
  // the block structure of the marginalization is the whole window's: which poses its frame-0 landmarks reach
  c->shard_kmax0 = 0;
  for (int l = 0; l < in->num_landmarks; l++)
    if (in->start_frame[l] == 0) c->shard_kmax0 = std::max(c->shard_kmax0, in->obs_offset[l + 1] - in->obs_offset[l]);
  int rc = reserve(c, 1, n, o1 - o0);
  if (rc) return rc;
  UploadMode mode;
  mode.sharded = (add_pose_side & 4) ? 2 : 1;
  mode.pose_side = (add_pose_side & 3) == 2 ? 2 : (add_pose_side & 3) ? 1 : 0;
  if ((rc = upload_window(c, 0, &sub, mode))) return rc;
  launch_setup(c, route_for(c, 1, MODE_SOLVE), MODE_SOLVE);  // (no Wt clear: a rank's share carries no LinwPlan)
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->shard_active = true;
  c->shard_begin = lm_begin, c->shard_end = lm_end;
  c->shard_state = 0;
  return LFVIO_OK;
}

// The synchronous phases: lfvio_shard_enqueue's phase, then a wait for it
static int shard_phase_sync(lfvio_ctx *c, int phase) {
  if (int rc = lfvio_shard_enqueue(c, phase)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 1;
}

// returns 1 when the caller must all-reduce the whole exchange buffer, 0 when nothing was produced
int lfvio_shard_linearize(lfvio_ctx *c) {
  if (!c || !c->shard_active) return LFVIO_ERR_ARG;
  if (c->shard_state != 0) return 0;
  return shard_phase_sync(c, 0);
}

// returns 1 when the caller must all-reduce the 16-scalar tail
int lfvio_shard_solve(lfvio_ctx *c) {
  if (!c || !c->shard_active) return LFVIO_ERR_ARG;
  if (c->shard_state != 0) return 0;
  return shard_phase_sync(c, 1);
}

int lfvio_shard_candidate(lfvio_ctx *c) {
  if (!c || !c->shard_active) return LFVIO_ERR_ARG;
  return shard_phase_sync(c, 2);
}

// *state: 0 = linearize next, 1 = step rejected: only a new candidate is needed, 2 = terminated
int lfvio_shard_decide(lfvio_ctx *c, int *state) {
  if (!c || !c->shard_active || !state) return LFVIO_ERR_ARG;
  hipLaunchKernelGGL(k_decide, dim3(1, 1), dim3(64), 0, c->stream, c->d_base, c->L.total);
  HIPCHK(c, hipGetLastError());
  TRState *tr = (TRState *)c->h_down.get();
  HIPCHK(c, hipMemcpyAsync(tr, c->d_base + offsetof(Slot, tr), offsetof(TRState, it), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (tr->done) c->shard_state = 2;
  else if (tr->do_lin || tr->do_schur) c->shard_state = 0;
  else c->shard_state = 1;
  *state = c->shard_state;
  return tr->error ? tr->error : LFVIO_OK;
}

// ---- stream-ordered driver: nothing but enqueues between the collectives ---------------------------------------------
// The phase functions above synchronize the stream four times per iteration so that the caller may run its collective
// from the host.  RCCL (and torch.distributed on it) is stream-ordered, so the loop needs none of that: the caller makes
// the context's stream its current one (torch.cuda.ExternalStream(lfvio_stream())), and per pass enqueues
//     lfvio_shard_enqueue(0); all_reduce(buf);  lfvio_shard_enqueue(1); all_reduce(tail);
//     lfvio_shard_enqueue(2); all_reduce(tail); lfvio_shard_enqueue(3);
// Every kernel tests the trust-region flags on the device, so a pass is the same sequence of calls whatever the loop
// decides (a rejected step re-linearizes nothing, a finished loop does nothing), which is also what makes the pattern
// of collectives identical on every rank without a broadcast.  Phase 3 copies the 16 flag words of the slot into a ring
// of pinned records; lfvio_shard_poll() waits for the OLDEST outstanding record, so the caller can keep one pass in
// flight behind the decision it is looking at (the pass in flight turns into no-ops if that decision was `done`).
// A collective over a buffer nobody refreshed must reproduce it: in such a pass k_sum zeroes the exchange buffer on every rank
// but the pose-side one, so the sum is the pose-side rank's (already reduced) copy, bit for bit.

int lfvio_shard_restart(lfvio_ctx *c) {  // the resident shard again from its uploaded state: no copy, one launch
  if (!c || !c->d_base || !c->info[0].resident) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  // decision records still outstanding (a run that ended on an error): their copies must have landed before the ring is reused
  for (; c->flag_tail < c->flag_head; c->flag_tail++) HIPCHK(c, hipEventSynchronize(c->flag_event[c->flag_tail % lfvio_ctx::FLAG_RING]));
  launch_setup(c, route_for(c, 1, MODE_SOLVE), MODE_SOLVE);
  HIPCHK(c, hipGetLastError());
  c->shard_active = true;
  c->shard_state = 0;
  c->flag_head = c->flag_tail = 0;
  return LFVIO_OK;
}

int lfvio_shard_enqueue(lfvio_ctx *c, int phase) {
  if (!c || !c->shard_active || phase < 0 || phase > 4) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);  // a group drives several devices from one thread
  const Route r = route_for(c, 1, MODE_SOLVE);
  const size_t st = c->L.total;
  switch (phase) {
    case 0:  // the shard's sweep (route_for) — either way the sums land in the exchange buffer
      launch_sweep(c, r, MODE_SOLVE, true);
      if (c->shard_group) {  // lfvio_group: what lets every rank form the Gauss-Newton step's landmark norms itself (k_lm_cb2)
        hipLaunchKernelGGL(k_lm_cb2, dim3(XP_WGS, 1), dim3(256), 0, c->stream, c->d_base, st);
      }
      break;
    case 1:
      shard_solve(c, r);
      hipLaunchKernelGGL(k_xpack, dim3(1, 1), dim3(256), 0, c->stream, c->d_base, st, 2);
      break;
    case 4:  // phases 1 and 2 as one, the scalars of both in ONE all-reduce (lfvio_group: the window was uploaded with bit 2 of add_pose_side)
      shard_solve(c, r);
      shard_candidate(c, r.g);
      hipLaunchKernelGGL(k_xpack, dim3(1, 1), dim3(256), 0, c->stream, c->d_base, st, 6);
      break;
    case 2:
      shard_candidate(c, r.g);
      hipLaunchKernelGGL(k_xpack, dim3(1, 1), dim3(256), 0, c->stream, c->d_base, st, 3);
      break;
    case 3:
    default: {
      if (c->flag_head - c->flag_tail >= lfvio_ctx::FLAG_RING) {
        c->err = "more than FLAG_RING decisions in flight: poll first";
        return LFVIO_ERR_ARG;
      }
      if (!c->h_flags) {  // the ring and its four events, or (a failure) neither
        MEMCHK(c, c->h_flags.reserve(sizeof(int) * 16 * lfvio_ctx::FLAG_RING), "hipHostMalloc((void **)&c->h_flags, sizeof(int) * 16 * lfvio_ctx::FLAG_RING, hipHostMallocDefault)");
        hipError_t made = hipSuccess;
        for (auto &e : c->flag_event)
          if (made == hipSuccess) made = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        for (auto &e : c->flag_event)
          if (made != hipSuccess && e) (void)hipEventDestroy(e), e = nullptr;
        if (made != hipSuccess) (void)c->h_flags.reset();
        HIPCHK_AS(c, made, "hipEventCreateWithFlags(&e, hipEventDisableTiming)");
      }
      hipLaunchKernelGGL(k_decide, dim3(1, 1), dim3(64), 0, c->stream, c->d_base, st);
      const int slot = c->flag_head % lfvio_ctx::FLAG_RING;
      HIPCHK(c, hipMemcpyAsync(c->h_flags + 16 * slot, c->d_base + offsetof(Slot, tr) + offsetof(TRState, iteration), sizeof(int) * 16,
                               hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipEventRecord(c->flag_event[slot], c->stream));
      c->flag_head++;
    }
  }
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

// *state as lfvio_shard_decide: 0 = linearize next, 1 = step rejected, 2 = terminated; returns 1 when a record was consumed,
// 0 when none is outstanding
int lfvio_shard_poll(lfvio_ctx *c, int *state) {
  if (!c || !c->shard_active || !state) return LFVIO_ERR_ARG;
  if (c->flag_tail == c->flag_head) return 0;
  const int slot = c->flag_tail % lfvio_ctx::FLAG_RING;
  HIPCHK(c, hipEventSynchronize(c->flag_event[slot]));
  c->flag_tail++;
  const int *f = c->h_flags + 16 * slot;  // TRHead's int block: iteration cur do_lin do_schur done ... error at [14]
  if (f[4]) c->shard_state = 2;
  else if (f[2] || f[3]) c->shard_state = 0;
  else c->shard_state = 1;
  *state = c->shard_state;
  if (f[14]) return f[14];
  return 1;
}

// ---- marginalization of the sharded window (after the loop has terminated, before lfvio_shard_finish)
//   E  gauge fix (double2vector / vector2double: identical on every rank), then the marginalization sweep over the
//      rank's own frame-0 landmarks, IMU factor 0 and the prior on the pose-side rank
//      -> [H_pp | g_p | Schur sums | N0]                                              --- sum-all-reduce (151 KB) ---
//   F  every rank eliminates the landmarks and eigen-decomposes the identical dense system -> identical prior
// returns 1 when the caller must all-reduce the whole exchange buffer
// enqueue only (the stream-ordered drivers: group.inc)
static int shard_marg_enqueue_linearize(lfvio_ctx *c, int flag) {
  if (!c || !c->shard_active || (flag != LFVIO_MARGIN_OLD && flag != LFVIO_MARGIN_SECOND_NEW)) return LFVIO_ERR_ARG;
  if (c->shard_state != 2) {
    c->err = "the sharded solve has not terminated";
    return LFVIO_ERR_ARG;
  }
  (void)hipSetDevice(c->device);
  const Route r = route_for(c, 1, MODE_MARG + flag);  // (the roles: k_linb sweeps the solve passes only)
  hipLaunchKernelGGL(k_gauge, dim3(1 + (r.g.lm + 1) / 2, 1), dim3(128), 0, c->stream, c->d_base, c->L.total, 0);
  launch_sweep(c, r, MODE_MARG + flag, true);
  HIPCHK(c, hipGetLastError());
  c->shard_state = 3;
  return 1;
}
static int shard_marg_enqueue_finish(lfvio_ctx *c, int flag) {
  if (!c || !c->shard_active || c->shard_state != 3) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  hipLaunchKernelGGL(k_marg_solve<false>, dim3(1, 1), dim3(MARG_THREADS), MARG_LDS, c->stream, c->d_base, c->L.total, flag);
  HIPCHK(c, hipGetLastError());
  c->shard_state = 2;
  return LFVIO_OK;
}

int lfvio_shard_marg_linearize(lfvio_ctx *c, int flag) {
  const int rc = shard_marg_enqueue_linearize(c, flag);
  if (rc < 0) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 1;
}

int lfvio_shard_marg_finish(lfvio_ctx *c, int flag, LfvioPrior *out) {
  if (!out) return LFVIO_ERR_ARG;
  const int rc = shard_marg_enqueue_finish(c, flag);
  if (rc < 0) return rc;
  return download_prior(c, 0, out);
}

// pose-side state is replicated; out->inv_depth receives only this rank's landmark range
// (after lfvio_shard_marg_linearize: the state after the gauge fix, i.e. what the next vector2double() holds)
int lfvio_shard_finish(lfvio_ctx *c, LfvioSolution *out) {
  if (!c || !c->shard_active || !out) return LFVIO_ERR_ARG;
  double *all = out->inv_depth;
  out->inv_depth = all ? all + c->shard_begin : nullptr;
  int rc = download_solution(c, 0, out);
  out->inv_depth = all;
  c->shard_active = false;
  return rc;
}
