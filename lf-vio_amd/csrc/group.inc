// group.inc — the multi-GPU entry points behind the C-ABI (SURVEY.md §8b `lfvio_create(int device_mask)`, §8e; included
// inside extern "C").  The host side is C++ and the collective is RCCL, called directly:
//   lfvio_group_create(mask)        one process, one context + stream per device of the mask, ncclCommInitAll
//   lfvio_group_create_rank(...)    one process per GPU (torchrun / mpirun launch), ncclCommInitRank from a 128-byte id the
//                                   launcher broadcasts
//   lfvio_group_create_local(...)   several shards on ONE device with a device-side sum in rank order instead of RCCL
//                                   (what the -m gpu tests use to play 2 / 4 / 8 ranks on the one GPU a test box has)
// A group runs the landmark-sharded optimization() of ONE window (BASELINE configs[3]) — lfvio_group_solve() is the call
// a re-implemented Estimator::optimization() body makes at estimator.cpp:484 instead of lfvio_solve() + lfvio_marginalize()
// — and splits independent resident windows over its devices (configs[4], no collective).
//
// RCCL is not a link dependency of the library (a single-GPU caller never loads it): librccl is dlopen()ed when the
// first group is created.  A process that already maps an RCCL (PyTorch ships its own copy) gets THAT one, so that one
// RCCL runtime serves the process.
// (<dlfcn.h> and <rccl/rccl.h> — types only — are included at the top of lfvio_hip.hip, outside extern "C")

namespace {

struct RcclApi {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string err, path;
};

RcclApi *rccl_api() {
  static RcclApi api;
  if (api.handle || !api.err.empty()) return &api;
  std::vector<std::string> cand;
  // LFVIO_RCCL_LIB overrides the search (lfvio.h): when it is set, that path is the only candidate
  const char *forced = getenv("LFVIO_RCCL_LIB");
  if (forced && forced[0]) cand.push_back(forced);
  else {
    // an RCCL the process has mapped already (torch/lib/librccl.so has no soname: found by path)
    FILE *f = fopen("/proc/self/maps", "r");
    if (f) {
      char line[1024];
      while (fgets(line, sizeof line, f)) {
        const char *p = strstr(line, "/");
        if (p && strstr(p, "librccl.so")) {
          std::string s(p);
          while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
          if (std::find(cand.begin(), cand.end(), s) == cand.end()) cand.push_back(s);
        }
      }
      fclose(f);
    }
    cand.push_back("librccl.so.1");
    cand.push_back("/opt/rocm/lib/librccl.so.1");
    cand.push_back("librccl.so");
  }
  std::string why;
  for (const std::string &p : cand) {
    api.handle = dlopen(p.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (api.handle) {
      api.path = p;
      break;
    }
    const char *e = dlerror();  // (once: the call clears the pending error)
    if (why.empty() && e) why = e;
  }
  if (!api.handle) {
    api.err = std::string("librccl not found (set LFVIO_RCCL_LIB): ") + why;
    return &api;
  }
#define LFVIO_SYM(field, name)                                               \
  api.field = (decltype(api.field))dlsym(api.handle, name);                  \
  if (!api.field) api.err = std::string("librccl: missing symbol ") + name
  LFVIO_SYM(GetUniqueId, "ncclGetUniqueId");
  LFVIO_SYM(CommInitRank, "ncclCommInitRank");
  LFVIO_SYM(CommInitAll, "ncclCommInitAll");
  LFVIO_SYM(CommDestroy, "ncclCommDestroy");
  LFVIO_SYM(AllReduce, "ncclAllReduce");
  LFVIO_SYM(AllGather, "ncclAllGather");
  LFVIO_SYM(GroupStart, "ncclGroupStart");
  LFVIO_SYM(GroupEnd, "ncclGroupEnd");
  LFVIO_SYM(GetErrorString, "ncclGetErrorString");
#undef LFVIO_SYM
  return &api;
}

// contiguous landmark ranges with ~equal observation counts (the sweep costs per observation); empty ranges are legal
void partition_landmarks(const int *obs_offset, int N, int world, std::vector<int> &cuts) {
  cuts.assign(world + 1, 0);
  const long long M = N > 0 ? obs_offset[N] : 0;
  for (int r = 1; r < world; r++) {
    const double target = (double)M * r / world;
    int c = (int)(std::lower_bound(obs_offset, obs_offset + N, target, [](int v, double t) { return (double)v < t; }) - obs_offset);
    cuts[r] = std::min(std::max(c, cuts[r - 1]), N);
  }
  cuts[world] = N;
}

constexpr int LOCAL_AR_MAX = 16;
struct LocalArArgs {
  double *buf[LOCAL_AR_MAX];
  int n;
};
// What a collective of the sharded loop carries: up to three ranges of the exchange buffer.
//   the reduced system   only what shards over landmarks — the camera part of H_pp (the packed prefix: rows < 73), the camera part
//                        of g_p, the Schur sums, the 16 scalars behind them and the 256 partials of k_lm_cb2: 2 701 + 73 + 4 112 doubles = 55 KB.  The speed / bias
//                        rows (IMU factors, prior) are evaluated on every rank — replicated, identical bits — and never travel
//                        (Slot::pose_side 2, kernels_lin.h pose_terms_here); round 4 sent the whole 151 KB buffer;
//   the scalars          the 16-scalar tail.
struct XRanges {
  int n, off[3], count[3];
  __host__ __device__ int total() const { return count[0] + (n > 1 ? count[1] : 0) + (n > 2 ? count[2] : 0); }
};
constexpr XRanges XR_SYSTEM = {3, {XOFF_H, XOFF_G, XOFF_S}, {SUM_VIS_PACKED, KC, SCHUR_LEN + 16 + 2 * XP_WGS}};
constexpr XRanges XR_SCALARS = {1, {XOFF_C, 0, 0}, {16, 0, 0}};
static_assert(XOFF_S + SCHUR_LEN == XOFF_C && XOFF_C + 16 == XCH_LEN && XOFF_P == XCH_LEN, "the scalars sit behind the Schur sums, k_lm_cb2's partials behind them");
// sum-all-reduce between the shards of a local group: every buffer <- the sum in rank order (deterministic)
__global__ __launch_bounds__(256) void k_local_allreduce(LocalArArgs a, XRanges xr) {
  int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= xr.total()) return;
  int off = xr.off[0];
  if (e >= xr.count[0]) {
    e -= xr.count[0], off = xr.off[1];
    if (e >= xr.count[1]) e -= xr.count[1], off = xr.off[2];
  }
  double s = a.buf[0][off + e];
  for (int r = 1; r < a.n; r++) s += a.buf[r][off + e];
  for (int r = 0; r < a.n; r++) a.buf[r][off + e] = s;
}

}  // namespace

struct lfvio_group {
  enum Backend { RCCL, LOCAL } backend = RCCL;
  int world = 1, rank0 = 0;          // ranks overall; rank of ctx[0]
  std::vector<lfvio_ctx *> ctx;      // the contexts of this process (ranks rank0 .. rank0 + ctx.size() - 1)
  std::vector<ncclComm_t> comm;      // RCCL: one communicator per local context
  std::vector<hipEvent_t> ev;        // LOCAL: one event per context + one "sum done"
  std::string err;
  // the resident sharded window
  bool uploaded = false, armed = false;
  int N = 0, M = 0, max_iter = 0;
  std::vector<int> cuts;
  DevBuf<double> d_gather;           // rank mode: inverse depths of all ranks, padded to equal counts (ncclAllGather)
  int last_passes = 0, last_collectives = 0;
  bool force_collective = false;
  std::vector<char> failed;          // local contexts that failed in the running call: they enqueue nothing more, but every collective goes out
  int inject_ctx = -1, inject_pass = -1, inject_phase = -1;  // lfvio_debug_group_inject_failure (tests)
  PinBuf<double> h_one;              // pinned 1.0: what a failed rank writes into XS_ERR in front of every collective it still issues
  // independent windows split over the devices: slot s -> context s % L, local slot s / L
  int batch = 0;
};

namespace {

int group_fail(lfvio_group *g, int rc, const std::string &what) {
  g->err = what;
  return rc;
}
#define NCCLCHK(g, call)                                                                            \
  do {                                                                                              \
    ncclResult_t r_ = (call);                                                                       \
    if (r_ != ncclSuccess) return group_fail(g, LFVIO_ERR_DEVICE, std::string(#call) + ": " + rccl_api()->GetErrorString(r_)); \
  } while (0)
#define GHIP(g, call) GHIP_AS(g, call, #call)
#define GHIP_AS(g, call, text)                                                                      \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) return group_fail(g, LFVIO_ERR_DEVICE, std::string(text) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define GMEM(g, ok, text) GHIP_AS(g, (ok) ? hipSuccess : hipPeekAtLastError(), text)  // (as MEMCHK)
#define GCTX(g, i, call)                                                                            \
  do {                                                                                              \
    int rc_ = (call);                                                                               \
    if (rc_ < 0) return group_fail(g, rc_, std::string(#call) + ": " + (g)->ctx[i]->err);          \
  } while (0)

// sum-all-reduce of the ranges `xr` of every rank's exchange buffer, ordered on each context's own stream: ONE collective (the
// RCCL calls of the ranges and of the local contexts inside one ncclGroupStart / End: one fused launch per device).
// A local context that failed earlier in the call still takes part — its peers are waiting in this collective — with XS_ERR
// raised in its scalars, which every rank's k_decide reads behind the reduction (kernels_solve.h decide_body).
int group_allreduce(lfvio_group *g, const XRanges &xr) {
  // a group of ONE rank has nothing to exchange: the sum is the buffer itself (LFVIO_GROUP_FORCE_COLLECTIVE=1 issues the
  // ncclAllReduce all the same — what the mask-of-one test runs, so that the RCCL path executes on a one-GPU box)
  if (g->world == 1 && !g->force_collective) return LFVIO_OK;
  g->last_collectives++;
  const int L = (int)g->ctx.size();
  for (int i = 0; i < L; i++)
    if (!g->failed.empty() && g->failed[i]) {
      lfvio_ctx *c = g->ctx[i];
      GHIP(g, hipSetDevice(c->device));
      if (!g->h_one) {
        GMEM(g, g->h_one.reserve(sizeof(double)), "hipHostMalloc((void **)&g->h_one, sizeof(double), hipHostMallocDefault)");
        *g->h_one = 1.0;
      }
      GHIP(g, hipMemcpyAsync(c->d_base + c->L.xch + (size_t)(XOFF_C + XS_ERR) * 8, g->h_one, sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
  if (g->backend == lfvio_group::LOCAL) {
    if (L == 1) return LFVIO_OK;
    LocalArArgs a;
    a.n = L;
    for (int i = 0; i < L; i++) {
      a.buf[i] = (double *)(g->ctx[i]->d_base + g->ctx[i]->L.xch);
      if (i > 0) {
        GHIP(g, hipEventRecord(g->ev[i], g->ctx[i]->stream));
        GHIP(g, hipStreamWaitEvent(g->ctx[0]->stream, g->ev[i], 0));
      }
    }
    hipLaunchKernelGGL(k_local_allreduce, dim3((xr.total() + 255) / 256), dim3(256), 0, g->ctx[0]->stream, a, xr);
    GHIP(g, hipGetLastError());
    GHIP(g, hipEventRecord(g->ev[L], g->ctx[0]->stream));
    for (int i = 1; i < L; i++) GHIP(g, hipStreamWaitEvent(g->ctx[i]->stream, g->ev[L], 0));
    return LFVIO_OK;
  }
  RcclApi *api = rccl_api();
  const bool grouped = L > 1 || xr.n > 1;
  if (grouped) NCCLCHK(g, api->GroupStart());
  for (int i = 0; i < L; i++) {
    lfvio_ctx *c = g->ctx[i];
    GHIP(g, hipSetDevice(c->device));
    for (int k = 0; k < xr.n; k++) {
      double *buf = (double *)(c->d_base + c->L.xch) + xr.off[k];
      NCCLCHK(g, api->AllReduce(buf, buf, (size_t)xr.count[k], ncclDouble, ncclSum, g->comm[i], c->stream));
    }
  }
  if (grouped) NCCLCHK(g, api->GroupEnd());
  return LFVIO_OK;
}

lfvio_group *group_alloc(const std::vector<int> &devices) {
  lfvio_group *g = new lfvio_group();
  if (const char *e = getenv("LFVIO_GROUP_FORCE_COLLECTIVE")) g->force_collective = e[0] == '1';
  for (int d : devices) {
    lfvio_ctx *c = lfvio_create(d);
    if (!c) {
      for (lfvio_ctx *p : g->ctx) lfvio_destroy(p);
      delete g;
      return nullptr;
    }
    g->ctx.push_back(c);
  }
  return g;
}

}  // namespace

lfvio_group *lfvio_group_create(unsigned device_mask) {
  std::vector<int> devs;
  for (int d = 0; d < 32; d++)
    if (device_mask & (1u << d)) devs.push_back(d);
  if (devs.empty()) return nullptr;
  lfvio_group *g = group_alloc(devs);  // (first: without a usable device nothing else is attempted)
  if (!g) return nullptr;
  RcclApi *api = rccl_api();
  if (!api->err.empty()) {
    fprintf(stderr, "lfvio_group_create: %s\n", api->err.c_str());
    lfvio_group_destroy(g);
    return nullptr;
  }
  g->backend = lfvio_group::RCCL;
  g->world = (int)devs.size();
  g->comm.assign(devs.size(), nullptr);
  const ncclResult_t r = api->CommInitAll(g->comm.data(), (int)devs.size(), devs.data());
  if (r != ncclSuccess) {
    fprintf(stderr, "lfvio_group_create: ncclCommInitAll: %s\n", api->GetErrorString(r));
    g->comm.clear();
    lfvio_group_destroy(g);
    return nullptr;
  }
  return g;
}

int lfvio_group_unique_id(char id[LFVIO_UNIQUE_ID_BYTES]) {
  static_assert(LFVIO_UNIQUE_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  RcclApi *api = rccl_api();
  if (!api->err.empty() || !id) return LFVIO_ERR_DEVICE;
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return LFVIO_ERR_DEVICE;
  std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return LFVIO_OK;
}

lfvio_group *lfvio_group_create_rank(int device, int rank, int world, const char id[LFVIO_UNIQUE_ID_BYTES]) {
  if (world < 1 || rank < 0 || rank >= world || !id) return nullptr;
  lfvio_group *g = group_alloc({device});
  if (!g) return nullptr;
  RcclApi *api = rccl_api();
  if (!api->err.empty()) {
    fprintf(stderr, "lfvio_group_create_rank: %s\n", api->err.c_str());
    lfvio_group_destroy(g);
    return nullptr;
  }
  g->backend = lfvio_group::RCCL;
  g->world = world, g->rank0 = rank;
  g->comm.assign(1, nullptr);
  ncclUniqueId u;
  std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  (void)hipSetDevice(device);
  const ncclResult_t r = api->CommInitRank(&g->comm[0], world, u, rank);
  if (r != ncclSuccess) {
    fprintf(stderr, "lfvio_group_create_rank: ncclCommInitRank: %s\n", api->GetErrorString(r));
    g->comm.clear();
    lfvio_group_destroy(g);
    return nullptr;
  }
  return g;
}

lfvio_group *lfvio_group_create_local(int device, int shards) {
  if (shards < 1 || shards > LOCAL_AR_MAX) return nullptr;
  lfvio_group *g = group_alloc(std::vector<int>(shards, device));
  if (!g) return nullptr;
  g->backend = lfvio_group::LOCAL;
  g->world = shards;
  g->ev.assign(shards + 1, nullptr);
  for (auto &e : g->ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      lfvio_group_destroy(g);
      return nullptr;
    }
  return g;
}

void lfvio_group_destroy(lfvio_group *g) {
  if (!g) return;
  for (size_t i = 0; i < g->comm.size(); i++)
    if (g->comm[i]) {
      (void)hipSetDevice(g->ctx[i]->device);
      (void)hipStreamSynchronize(g->ctx[i]->stream);
      (void)rccl_api()->CommDestroy(g->comm[i]);
    }
  for (auto &e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->d_gather) (void)hipSetDevice(g->ctx[0]->device);
  const std::vector<lfvio_ctx *> ctx = std::move(g->ctx);
  delete g;  // its buffers, before the contexts
  for (lfvio_ctx *c : ctx) lfvio_destroy(c);
}

const char *lfvio_group_last_error(const lfvio_group *g) { return g ? g->err.c_str() : "null group"; }
int lfvio_group_size(const lfvio_group *g) { return g ? g->world : 0; }
int lfvio_group_local(const lfvio_group *g) { return g ? (int)g->ctx.size() : 0; }
int lfvio_group_rank(const lfvio_group *g) { return g ? g->rank0 : -1; }
lfvio_ctx *lfvio_group_ctx(lfvio_group *g, int i) { return (g && i >= 0 && i < (int)g->ctx.size()) ? g->ctx[i] : nullptr; }
const char *lfvio_group_backend(const lfvio_group *g) {
  if (!g) return "";
  return g->backend == lfvio_group::LOCAL ? "local" : rccl_api()->path.c_str();
}

// ---- ONE window, landmark-sharded over the ranks of the group --------------------------------------------------------
// Every rank is handed the same window; rank r keeps the landmark range cuts[r] .. cuts[r + 1] (balanced on observation
// count), the pose-side factors (IMU, prior) live on rank 0.
int lfvio_group_upload(lfvio_group *g, const LfvioWindow *in) {
  if (!g || !in) return LFVIO_ERR_ARG;
  if (in->num_landmarks < 0 || (in->num_landmarks > 0 && !in->obs_offset)) return group_fail(g, LFVIO_ERR_ARG, "null window arrays");
  partition_landmarks(in->obs_offset, in->num_landmarks, g->world, g->cuts);
  g->uploaded = false;
  for (size_t i = 0; i < g->ctx.size(); i++) {
    const int r = g->rank0 + (int)i;
    // (rank 0 adds the pose-side factors everywhere; the others evaluate them too and keep them in the rows that do not travel: 2)
    GCTX(g, i, lfvio_shard_begin(g->ctx[i], in, g->cuts[r], g->cuts[r + 1], (r == 0 ? 1 : 2) | 4));  // | 4: two collectives per pass (lfvio_shard_enqueue phase 4)
  }
  g->N = in->num_landmarks, g->M = in->num_observations, g->max_iter = in->max_num_iterations;
  g->uploaded = true, g->armed = true;
  return LFVIO_OK;
}

// The whole optimization() of the resident window: trust-region loop, then (marg_flag >= 0) the gauge fix of
// double2vector() and the marginalization.  Stream-ordered: between the collectives nothing but enqueues, one pass kept in
// flight behind the decision being read (shard.inc); the call returns with every stream idle.
int lfvio_group_optimize(lfvio_group *g, int marg_flag) {
  if (!g || !g->uploaded) return LFVIO_ERR_ARG;
  if (marg_flag >= 0 && marg_flag != LFVIO_MARGIN_OLD && marg_flag != LFVIO_MARGIN_SECOND_NEW) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size();
  if (!g->armed)
    for (int i = 0; i < L; i++) GCTX(g, i, lfvio_shard_restart(g->ctx[i]));
  g->armed = false;
  g->last_passes = g->last_collectives = 0;
  const int limit = 4 * (g->max_iter + 8);
  // A local failure (an enqueue refused, a HIP error) must not leave the peers of the group waiting in a collective this rank
  // never enters: the context is marked, enqueues nothing more, and the call goes on issuing EVERY collective of the sequence —
  // with XS_ERR raised in that context's scalars — until the pass in which all ranks read the flag behind a reduction (k_decide)
  // and end their loops together; then the first error is returned.
  g->failed.assign(L, 0);
  int first_rc = LFVIO_OK, fail_pass = -1;
  std::string first_err;
  auto fail_ctx = [&](int i, int rc, const std::string &what, bool before_last_collective) {
    g->failed[i] = 1;
    if (first_rc == LFVIO_OK) first_rc = rc, first_err = what, fail_pass = g->last_passes + (before_last_collective ? 0 : 1);
  };
  auto enqueue_all = [&](int phase) {
    for (int i = 0; i < L; i++) {
      if (g->failed[i]) continue;
      int rc = lfvio_shard_enqueue(g->ctx[i], phase);
      if (rc >= 0 && i == g->inject_ctx && g->last_passes == g->inject_pass && phase == g->inject_phase) rc = LFVIO_ERR_DEVICE, g->ctx[i]->err = "injected failure (lfvio_debug_group_inject_failure)";
      if (rc < 0) fail_ctx(i, rc, std::string("lfvio_shard_enqueue: ") + g->ctx[i]->err, phase != 3);
    }
  };
  // (a collective that cannot be issued at all — RCCL itself failed — is the one error nothing can be done about)
  auto one_pass = [&]() -> int {
    int rc;
    enqueue_all(0);  // the sweep of the rank's landmarks
    if ((rc = group_allreduce(g, XR_SYSTEM))) return rc;
    enqueue_all(4);  // solve, back-substitution, candidate (the Gauss-Newton step until k_decide has its norm), its cost
    if ((rc = group_allreduce(g, XR_SCALARS))) return rc;
    enqueue_all(3);  // the decision, identical on every rank
    g->last_passes++;
    return LFVIO_OK;
  };
  // the decision records of the local contexts are identical (every rank solves the identical reduced system)
  // A context that failed still holds the decisions of the passes it enqueued BEFORE it failed — the group's decisions, identical on
  // every rank — and goes on reading them: with one process per GPU they are the only way this rank learns that the loop has
  // terminated in a pass before the failure (ADVICE round 5: it would otherwise issue the collectives of one or two passes its
  // peers, already in the marginalization, never enter).
  auto poll = [&](int *state) -> int {
    int got = 0, ref = -1;
    for (int i = 0; i < L; i++) {
      if (g->failed[i] && g->ctx[i]->flag_tail == g->ctx[i]->flag_head) continue;
      int s = 0;
      const int rc = lfvio_shard_poll(g->ctx[i], &s);
      if (rc < 0 && g->failed[i]) continue;  // (a record that carries the error word is the failure's own, not a decision)
      if (rc < 0) return group_fail(g, rc, std::string("lfvio_shard_poll: ") + g->ctx[i]->err);
      if (ref < 0) ref = i, got = rc, *state = s;
      else if (rc != got || (rc == 1 && s != *state)) return group_fail(g, LFVIO_ERR_DEVICE, "the shards of the group disagree on the trust-region decision");
    }
    return got;
  };
  auto drain = [&]() {  // leave no record outstanding and no stream busy behind an error
    int s;
    for (int i = 0; i < L; i++)
      while (lfvio_shard_poll(g->ctx[i], &s) == 1) {
      }
  };
  int rc = one_pass();
  int state = 0;
  bool terminated = false;  // a decision read from a record says so: the peers have read the same one and left the loop with this pass in flight
  while (!rc) {
    if ((rc = one_pass())) break;
    const int got = poll(&state);
    if (got < 0) {
      rc = got;
      break;
    }
    if (got == 1 && state == 2) {
      terminated = true;
      break;
    }
    // every rank saw the flag of a failure in pass fail_pass behind that pass's last reduction and has one more pass in flight
    // behind it, like this one: the sequences of collectives end together
    if (first_rc != LFVIO_OK && g->last_passes >= fail_pass + 2) break;
    if (g->last_passes > limit) {
      rc = group_fail(g, LFVIO_ERR_DEVICE, "sharded loop did not terminate");
      break;
    }
  }
  // (a rank that failed in the no-op pass behind the terminating one goes on: its peers are on their way into the marginalization's
  // collective, which it enters with XS_ERR raised — and returns its error behind it)
  if (rc || (first_rc != LFVIO_OK && !(terminated && marg_flag >= 0))) {
    const std::string keep = first_rc != LFVIO_OK ? first_err : g->err;
    drain();
    for (int i = 0; i < L; i++) {
      (void)hipSetDevice(g->ctx[i]->device);
      (void)hipStreamSynchronize(g->ctx[i]->stream);
    }
    g->err = keep;
    return first_rc != LFVIO_OK ? first_rc : rc;
  }
  drain();  // the pass in flight behind the terminated loop was a no-op: its record
  if (marg_flag >= 0) {
    for (int i = 0; i < L; i++) {
      if (g->failed[i]) continue;
      const int mrc = shard_marg_enqueue_linearize(g->ctx[i], marg_flag);
      if (mrc < 0) fail_ctx(i, mrc, std::string("shard_marg_enqueue_linearize: ") + g->ctx[i]->err, true);
    }
    if ((rc = group_allreduce(g, XR_SYSTEM))) return rc;
    for (int i = 0; i < L; i++)
      if (!g->failed[i]) GCTX(g, i, shard_marg_enqueue_finish(g->ctx[i], marg_flag));
  }
  // (a peer that failed in the marginalization's sweep said so in that collective: the flag comes down with the final wait)
  double peer_err = 0.0;
  for (int i = 0; i < L; i++) {
    GHIP(g, hipSetDevice(g->ctx[i]->device));
    if (marg_flag >= 0 && i == 0 && (g->world > 1 || g->force_collective))
      GHIP(g, hipMemcpyAsync(&peer_err, g->ctx[0]->d_base + g->ctx[0]->L.xch + (size_t)(XOFF_C + XS_ERR) * 8, sizeof(double), hipMemcpyDeviceToHost, g->ctx[0]->stream));
    GHIP(g, hipStreamSynchronize(g->ctx[i]->stream));
  }
  if (first_rc != LFVIO_OK) return group_fail(g, first_rc, first_err);
  if (peer_err != 0.0) return group_fail(g, LFVIO_ERR_DEVICE, "a rank of the group failed in the marginalization (its error word arrived with the collective)");
  return LFVIO_OK;
}

// tests: the local context `local_ctx` reports a failure when it enqueues phase `phase` (0 .. 3) of pass `pass` of the next
// lfvio_group_optimize(); local_ctx < 0 clears it
int lfvio_debug_group_inject_failure(lfvio_group *g, int local_ctx, int pass, int phase) {
  if (!g) return LFVIO_ERR_ARG;
  g->inject_ctx = local_ctx, g->inject_pass = pass, g->inject_phase = phase;
  return LFVIO_OK;
}

// Results of the last lfvio_group_optimize(): the pose-side state is replicated (identical on every rank); sol->inv_depth
// [num_landmarks] is complete on every rank — gathered in-process from the local contexts, and with ncclAllGather between
// processes.  After a marginalization the state is the one after the gauge fix (what the next vector2double() holds).
int lfvio_group_download(lfvio_group *g, LfvioSolution *sol, LfvioPrior *prior) {
  if (!g || !g->uploaded) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size();
  if (prior) GCTX(g, 0, download_prior(g->ctx[0], 0, prior));
  if (!sol) return LFVIO_OK;
  double *all = sol->inv_depth;
  // One process per GPU: the gather below is a collective — every rank that asks for a solution takes part in it whether or
  // not it wants the inverse depths itself (its own range is what the others are waiting for): a scratch array stands in.
  std::vector<double> scratch_all;
  const bool gather = g->world > L && g->N > 0;
  if (gather && !all) scratch_all.resize((size_t)g->N), all = scratch_all.data();
  // pose-side state and the summary from the first local context; inverse depths: every local context its own range
  for (int i = L - 1; i >= 0; i--) {
    const int r = g->rank0 + i;
    if (i > 0) {
      if (!all || g->cuts[r + 1] == g->cuts[r]) continue;
      LfvioSolution tmp;
      tmp.inv_depth = all + g->cuts[r];
      GCTX(g, i, download_solution(g->ctx[i], 0, &tmp));
    } else {
      double *const asked = sol->inv_depth;
      sol->inv_depth = all ? all + g->cuts[r] : nullptr;
      const int rc = download_solution(g->ctx[0], 0, sol);
      sol->inv_depth = asked;
      if (rc < 0) return group_fail(g, rc, std::string("download_solution: ") + g->ctx[0]->err);
    }
  }
  if (gather) {
    // one process per GPU: ncclAllGather of the ranges, padded to the longest one
    RcclApi *api = rccl_api();
    int pad = 0;
    for (int r = 0; r < g->world; r++) pad = std::max(pad, g->cuts[r + 1] - g->cuts[r]);
    lfvio_ctx *c = g->ctx[0];
    GHIP(g, hipSetDevice(c->device));
    const size_t need = (size_t)pad * (g->world + 1) * sizeof(double);
    if (need > g->d_gather.capacity()) {
      GMEM(g, g->d_gather.reset(), "hipFree(g->d_gather)");
      GMEM(g, g->d_gather.reserve(need), "hipMalloc((void **)&g->d_gather, need)");
    }
    double *send = g->d_gather, *recv = g->d_gather + pad;
    const int b = g->cuts[g->rank0], n = g->cuts[g->rank0 + 1] - b;
    GHIP(g, hipMemsetAsync(send, 0, (size_t)pad * sizeof(double), c->stream));
    if (n) GHIP(g, hipMemcpyAsync(send, all + b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(g, api->AllGather(send, recv, (size_t)pad, ncclDouble, g->comm[0], c->stream));
    std::vector<double> host((size_t)pad * g->world);
    GHIP(g, hipMemcpyAsync(host.data(), recv, host.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GHIP(g, hipStreamSynchronize(c->stream));
    for (int r = 0; r < g->world; r++)
      std::memcpy(all + g->cuts[r], host.data() + (size_t)pad * r, (size_t)(g->cuts[r + 1] - g->cuts[r]) * sizeof(double));
  }
  return LFVIO_OK;
}

int lfvio_group_solve(lfvio_group *g, const LfvioWindow *in, int marg_flag, LfvioSolution *sol, LfvioPrior *prior) {
  int rc = lfvio_group_upload(g, in);
  if (rc) return rc;
  if ((rc = lfvio_group_optimize(g, marg_flag))) return rc;
  return lfvio_group_download(g, sol, marg_flag >= 0 ? prior : nullptr);
}

// doubles in the per-pass all-reduce of the reduced system (the scalar all-reduces carry 16)
int lfvio_group_payload_doubles(void) { return XR_SYSTEM.total(); }
int lfvio_group_last_passes(const lfvio_group *g) { return g ? g->last_passes : -1; }
int lfvio_group_last_collectives(const lfvio_group *g) { return g ? g->last_collectives : -1; }
int lfvio_group_range(const lfvio_group *g, int rank, int *begin, int *end) {
  if (!g || !g->uploaded || rank < 0 || rank >= g->world || !begin || !end) return LFVIO_ERR_ARG;
  *begin = g->cuts[rank], *end = g->cuts[rank + 1];
  return LFVIO_OK;
}

// ---- independent windows split over the devices of the group (BASELINE configs[4]; no data-path collective) ----------
int lfvio_group_batch_reserve(lfvio_group *g, int batch, int max_landmarks, int max_observations) {
  if (!g || batch <= 0) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size();
  for (int i = 0; i < L; i++) GCTX(g, i, lfvio_batch_reserve(g->ctx[i], (batch - i + L - 1) / L > 0 ? (batch - i + L - 1) / L : 1, max_landmarks, max_observations));
  g->batch = batch;
  return LFVIO_OK;
}
int lfvio_group_batch_upload(lfvio_group *g, int slot, const LfvioWindow *in) {
  if (!g || slot < 0 || slot >= g->batch) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size(), i = slot % L;
  GCTX(g, i, lfvio_batch_upload(g->ctx[i], slot / L, in));
  return LFVIO_OK;
}
// slots [0, count): every device enqueues its share, then every stream is waited for
int lfvio_group_batch_optimize(lfvio_group *g, int count, int marg_flag) {
  if (!g || count <= 0 || count > g->batch) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size();
  for (int i = 0; i < L; i++) {
    const int n = (count - i + L - 1) / L;
    if (n > 0) GCTX(g, i, lfvio_batch_optimize_async(g->ctx[i], n, marg_flag));
  }
  for (int i = 0; i < L; i++) GCTX(g, i, lfvio_batch_sync(g->ctx[i]));
  return LFVIO_OK;
}
int lfvio_group_batch_download(lfvio_group *g, int slot, LfvioSolution *sol, LfvioPrior *prior) {
  if (!g || slot < 0 || slot >= g->batch) return LFVIO_ERR_ARG;
  const int L = (int)g->ctx.size(), i = slot % L;
  GCTX(g, i, lfvio_batch_download(g->ctx[i], slot / L, sol, prior));
  return LFVIO_OK;
}
