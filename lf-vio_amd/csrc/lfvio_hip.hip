// lfvio_hip.hip — C-ABI implementation (include/lfvio.h) on HIP for gfx950 (MI355X).
//
// Host side of the hot path of LF-VIO's Estimator::optimization()
// (vins_estimator/src/estimator.cpp:676-1009): packs one LfvioWindow into the device
// layout of dev_types.h, launches the kernel pipeline and unpacks the result.
// There is NO CPU fallback: without a usable HIP device lfvio_create() fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
// The few RCCL types group.inc needs, declared here with the values of the public ABI (rccl.h: ncclSuccess = 0, ncclSum = 0,
// ncclDouble = 8, a 128-byte unique id): librccl is dlopen()ed by group.inc, not linked, and the single-GPU library builds on
// a ROCm install without the RCCL development headers.
typedef struct ncclComm *ncclComm_t;
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct {
  char internal[NCCL_UNIQUE_ID_BYTES];
} ncclUniqueId;
typedef int ncclResult_t;
typedef int ncclDataType_t;
typedef int ncclRedOp_t;
constexpr ncclResult_t ncclSuccess = 0;
constexpr ncclRedOp_t ncclSum = 0;
constexpr ncclDataType_t ncclDouble = 8;

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lfvio.h"
#include "../../include/lfvio_debug.h"
#include "kernels_marg.h"
#include "kernels_solve.h"
#include "kernels_feat.h"
#include "kernels_linw.h"
#include "linb_plan.h"
#include "call_state.h"
#include "kernels_stepw.h"
#include "kernels_relo.h"
#include "kernels_twoview.h"
#include "kernels_relpose.h"
#include "kernels_vialign.h"
#include "kernels_pnp.h"
#include "kernels_sfmba.h"
#include "kernels_sfmchain.h"
#include "kernels_klt.h"
#include "kernels_gft.h"
#include "kernels_clahe.h"
#include "kernels_imgfmt.h"
#include "kernels_remap.h"
#include "kernels_tracksource.h"
#include "tracksource_plan.h"
#include "kernels_fuse.h"
#include "kernels_track.h"
#include "kernels_trackframe.h"
#include "kernels_trackbatch.h"
#include "window_pack.h"
#include "dev_mem.h"

#define HIPCHK(ctx, call) HIPCHK_AS(ctx, call, #call)
#define HIPCHK_AS(ctx, call, text)                                                             \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (ctx)->err = std::string(text) + ": " + hipGetErrorString(e_);                           \
      return LFVIO_ERR_DEVICE;                                                                 \
    }                                                                                          \
  } while (0)
// a Buf's reserve() / reset() (dev_mem.h) under the text of the runtime call behind it, whose error is the runtime's last one
#define MEMCHK(ctx, ok, text) HIPCHK_AS(ctx, (ok) ? hipSuccess : hipPeekAtLastError(), text)

namespace {

// (Layout, make_layout and the kernels' SlotArgs: slot_args.h)

size_t down_bytes(int maxN) { return sizeof(FrameState) * 2 + sizeof(TRState) + 2 * ((size_t)maxN * 8 + 128) + sizeof(LfvioPrior) + 4096; }

struct SlotHostInfo {
  bool spec_on = false;  // Slot::spec_on of the resident window
  // The uploaded state holds a quaternion off the unit sphere (struct Tab, dev_types.h: |q|^2 further than TAB_OFF_SPHERE from 1): the
  // sweep that linearizes at that state — the first pass of a call — and, where the off-sphere quaternion is an extrinsic that is not
  // estimated, every sweep of the window run the instantiations that know the reference's two back-rotations
  bool offs_first = false, offs_all = false;
  int N = 0, M = 0, gLm = 0, gLw = 0, gCh = 0, gSc = 0;  // gLm: landmark blocks of 64; gLw: landmark workgroups of k_lin
  int marg_n = 0;            // the largest prior (tangent rows) a marginalization of this window can produce
  int prior_n = 0;           // rows of the uploaded window's input prior (0: none)
  int max_iter = 0;          // LfvioWindow::max_num_iterations of the uploaded window
  double max_seconds = -1.0;  // LfvioWindow::max_solver_time_in_seconds (<= 0: no cap)
  std::vector<int> perm;  // device order -> caller order
  bool linw_ok = false;    // the window carries a LinwPlan and its arrays (kernels_linw.h)
  bool linb_ok = false;    // ... as a group list: a large single window (k_linb)
  int linb_ng = 0;
  bool uploaded = false;   // the slot's work-array pointers are on the device (until the next reserve())
  bool resident = false;   // a window is resident: N, perm, grid sizes below describe what the device holds.  Cleared while an upload
                           // rewrites them and set again when its copies are enqueued, so a refused upload leaves a slot that every
                           // later call refuses instead of one described by the wrong sizes
  LfvioPrior in_prior;    // kept for the "prior passes through" case of MARGIN_SECOND_NEW
  bool has_in_prior = false;
  bool in_prior_device = false;  // ... whose values never came to the host (lfvio_batch_upload_chained_device): in_prior holds the structure only
  // what a marginalization of this window leaves as its prior, as planned at the upload [MARGIN_OLD, MARGIN_SECOND_NEW]: the
  // structure of the NEXT window's input prior when that window takes it over on the device
  struct MargOut {
    int valid = 0, n = 0, m = 0, nb = 0;
    int kind[LFVIO_MAX_PRIOR_BLOCKS], frame[LFVIO_MAX_PRIOR_BLOCKS], idx[LFVIO_MAX_PRIOR_BLOCKS];
  } marg_out[2];
  int mail_seq = 0;  // Slot::mail_seq of the resident window: what its mailbox flags are set to
  // k_sum's gather lists on the device are a function of the chunks per frame pair alone: kept from one upload of the slot
  // to the next while that table stays the same (consecutive windows of one estimator: nearly always).  WindowPacker::gather_lists
  // (window_pack.h) compares and replaces the key; upload_window sets list_items once the lists' copy is enqueued
  std::vector<int> list_key;  // pair_chunk0[0 .. NPAIR], pre_gram
  int list_items = -1;
};

struct Grid {
  int lm, ch, sc, lw;
  int ch_raw;  // largest chunk count of a slot before the rounding of `ch` (what decides the two-level sums: Slot::pre_gram, window_pack.h)
};

// k_setup's launch: grid.x and the bits of its last argument.  A resident batch is bound by the number of workgroups the launch
// dispatches (21 per window, 16 of them for a prior that ONE workgroup handles there: 10 752 workgroups for 512 windows, ~10 ns each),
// so it goes out with the compact grid — state, IMU roots, one prior workgroup, inverse depths — when every resident prior fits
// that workgroup's 4 x 4 tiling (n <= 88: kernels_lin.h).
struct SetupLaunch {
  int gx, bits;
};

// How a launch over the resident slots [0, count) linearizes, decided once (route_for) for every site that enqueues or reports it
struct Route {
  enum Sweep { ROLES = 0, LINW = 1, LINB = 2 } sweep;  // k_lin roles + k_sum | k_linw | k_linb + k_sumb (lfvio_debug_query "sweep_kernel")
  int count;
  Grid g;
  size_t role_wgs;    // workgroups of k_lin as one grid of all its roles
  bool split;         // k_lin goes out role by role (a resident batch)
  int linb_gx;        // grid.x of k_linb (LINB only)
  SetupLaunch setup;  // k_setup in front of the sweep
  int offs;           // slots_offs
};

// What a captured graph was built for: a graph whose key differs is captured again
struct GraphKey {
  int count = 0, lm = 0, ch = 0, sc = 0, sweep = -1, linb_gx = 0, offs = 0, setup = -1, spec = 0, passes = 0;
  bool operator==(const GraphKey &o) const {
    return count == o.count && lm == o.lm && ch == o.ch && sc == o.sc && sweep == o.sweep && linb_gx == o.linb_gx && offs == o.offs &&
           setup == o.setup && spec == o.spec && passes == o.passes;
  }
};

}  // namespace

// The streams and events of a context, as its base: ~lfvio_ctx frees every buffer (the members) before this destroys a stream
struct CtxQueues {
  hipStream_t stream = nullptr, fstream = nullptr;
  static constexpr int WORKERS = 2;  // two, so that the newest accepted state never waits for the round of an older one to notice it is stale
  hipStream_t sstream[WORKERS] = {};
  // the copies out of h_stage are awaited by the NEXT user of the staging block, not by the upload that enqueued them
  hipEvent_t stage_event = nullptr;
  static constexpr int FLAG_RING = 4;
  hipEvent_t flag_event[FLAG_RING] = {};  // all four, or none (shard.inc)
  ~CtxQueues() {
    for (auto &e : flag_event)
      if (e) (void)hipEventDestroy(e);
    if (stage_event) (void)hipEventDestroy(stage_event);
    if (fstream) (void)hipStreamDestroy(fstream);
    for (auto &st : sstream)
      if (st) (void)hipStreamDestroy(st);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// Every d_* (device) and h_* (pinned) block below is a Buf (dev_mem.h): owned here, grow-only, freed with the context.
struct lfvio_ctx : CtxQueues {
  int device = 0;
  DevBuf<char> d_feat;  // scratch of lfvio_triangulate / lfvio_shift_depth
  PinBuf<char> h_feat;  // pinned mirror of d_feat: the inputs of a feature step go up as ONE copy, its outputs come down as one
  // The single route's image stream (track_stream.h): which of each pair of buffers below is the resident one and what it holds.
  // Every separate tracker call and lfvio_track_frame move it; the buffers stay with the call that introduced them.
  TrackStream tstream;
  KbCache track_kb;  // the last KANNALA_BRANDT camera's monotone range (camera_kb.h), for every single-route call that takes a camera
  // lfvio_klt_track (klt.inc): two pyramid buffers of their own; tstream.pcur holds the resident image's levels 0 .. tstream.built
  struct KltState {
    DevBuf<unsigned char> d[2];
  } klt;
  // lfvio_gft_detect (gft.inc): the base mask (all 255 until lfvio_gft_set_mask; survives lfvio_klt_reset) and the work arrays of one
  // image size (lambda, final mask, candidates, kept pixels, GftDev)
  struct GftState {
    DevBuf<unsigned char> mask;
    DevBuf<char> work;
  } gft;
  // lfvio_clahe_set / lfvio_clahe_apply (clahe.inc): the setting (off after lfvio_create; survives lfvio_klt_reset) and the
  // [tiles][256] int table with the LUTs behind it, allocated at the first use; dirty: the table may hold counts
  struct ClaheState {
    bool on = false;
    LfvioClaheIn cfg = {};
    DevBuf<char> work;
    bool dirty = false;
  } clahe;
  // lfvio_image_format_set (imgfmt.inc): the encoding of the images the single route's calls take (off after lfvio_create; survives
  // lfvio_klt_reset and lfvio_track_frame_reset).  get(): what imgfmt_plan (image_format.h) takes
  struct ImageFormatState {
    bool on = false;
    LfvioImageFormat f = {};
    const LfvioImageFormat *get() const { return on ? &f : nullptr; }
  } imgfmt;
  // lfvio_remap_build / lfvio_remap_apply (remap.inc): what is resident (remap_plan.h), the two float maps [2][height][width] and the
  // integer map [height][width] in device memory of their own, allocated at the first build; kb: the last KANNALA_BRANDT projector's
  // monotone range.  No tracker call looks at any of it unless lfvio_track_source_set is on, and lfvio_klt_reset leaves it alone.
  struct RemapState {
    RemapResident r;
    DevBuf<float> map;
    DevBuf<int> index;
    KbCache kb;
  } remap;
  // lfvio_track_source_set (tracksource.inc): the single route's tracker calls take the SOURCE image and fill level 0 through the
  // resident map above (off after lfvio_create; survives lfvio_klt_reset, lfvio_track_frame_reset and lfvio_remap_reset)
  TrackSourceState tsource;
  // lfvio_track_undistort (track.inc): the (id, un_pts_3d) pairs of the previous call — [4096 ints | 4096 x 3 floats] twice, allocated
  // at the first use; tstream.mcur holds the tstream.mcount resident pairs (0: the map is empty), tstream.time is that call's
  struct TrackState {
    DevBuf<char> map[2];
  } track;
  // lfvio_track_frame (trackframe.inc): the track table — [4096 x 2 floats | 4096 ids | 4096 counts] twice, allocated at the first
  // use; tstream.tcur holds the tstream.count resident entries, tstream.n_id is the next id to hand out
  struct TrackFrameState {
    DevBuf<char> table[2];
  } tframe;
  // lfvio_track_batch_* (trackbatch.inc): `slot.size()` independent streams, each a TrackStream as the single route's.  fixed: per slot
  // two track tables and two maps (TB_FIXED_BYTES); image: per slot [pyramid | pyramid | base mask | detector's
  // arrays] with the capacities of `lay` (trackbatch_plan.h), allocated at the first frame or mask; clahe: per slot the int table and
  // the LUTs, allocated at the first frame with the setting on.  None of it is the single route's, and the single route's is none of it.
  struct TrackBatchState {
    std::vector<TrackStream> slot;
    std::vector<KbCache> kb;  // per slot: the slot's last KANNALA_BRANDT camera's monotone range (camera_kb.h)
    DevBuf<char> fixed, image, clahe;
    TbImage lay = {0, 0, 0};
    bool clahe_on = false, clahe_dirty = false;
    LfvioClaheIn cfg = {};
    ImageFormatState imgfmt;  // lfvio_track_batch_format: the batch's, one for every slot
    // lfvio_track_batch_map / lfvio_track_batch_source: per slot what its resident remap is, and the maps themselves —
    // per slot [map_x | map_y | integer map] with the capacities of `mlay`, allocated at the first build, grown for a larger output;
    // `indexed`: the ONE source geometry every mapped slot's integer map is written for.  None of it is RemapState's above.
    std::vector<TbMapInfo> map;
    DevBuf<char> maps;
    TbMaps mlay = {0};
    TbIndexed indexed;
    TrackSourceState source;  // lfvio_track_batch_source: the batch's, one for every slot; survives reserve and reset
    KbCache map_kb;
  } tbatch;
  std::string err;
  int batch = 0;
  Layout L;
  DevBuf<char> d_base;
  PinBuf<char> h_stage;  // one slot's header + inputs
  PinBuf<char> h_down;   // download buffer
  std::vector<SlotHostInfo> info;
  std::vector<int> perm_build;  // pack_window (window_pack.h) builds the next permutation here; commit_slot_info swaps it in
  // cached graph of the solve loop
  hipGraphExec_t graph = nullptr;
  GraphKey graph_key;
  // cached graph of one chunk of passes (synchronous entry points: the loop is launched chunk by chunk)
  // [publish]: the variants whose gated gauge fix / marginalization also push state and prior into the caller's mailbox
  // (CallPlan::publish)
  hipGraphExec_t chunk[2] = {}, tail[2][3] = {};  // chunk[speculation variant]
  hipGraphExec_t first[2][2][4][13] = {};  // [speculation variant: 0 three candidates (or none), 1 four][publish][0: solve only, 1 + flag: with the gated tail][passes in the first graph]
  int fixed_passes = 0;             // debug (lfvio_debug_configure "first_passes"): > 0 sizes every first graph with this many passes
  int recent_passes[4] = {0, 0, 0, 0}, recent_head = 0;  // passes of the last four synchronous calls (predict())
  int predict_passes = 4;           // passes the first graph of the next call carries: the most any of the last four calls needed (predict()); tail[flag]: force-done + gated gauge fix + marginalization
  double pass_seconds = 2e-4;       // measured duration of one pass of a continuation chunk (sizes the first graph of a call with a wall-clock cap)
  GraphKey chunk_key;  // of chunk, tail, first and the workers' graphs
  DevBuf<int> d_pending;  // number of slots whose trust-region loop is not done
  PinBuf<PendingBlock> h_pending;
  // lfvio_batch_optimize_begin / _finish: the solution of slot 0 arrives in host memory the gated gauge fix writes directly
  // (Slot::mail, dev_types.h MAIL_*) while the marginalization of the same graph is still running.  What is in flight then, and what
  // every entry point has to wait for, is `call` (call_state.h: the state table; join_inflight: every entry point that touches the
  // slots or the stream starts with it).  The landmark-parallel steps either side of optimization()
  // (triangulate / shift_depth / preintegrate) have their own stream and scratch and do not wait for the tail.
  CallState call;
  PinBuf<char, hipHostMallocMapped | hipHostMallocCoherent> h_mail;
  char *d_mail = nullptr;  // h_mail in the device's address space
  // The marginalization run ahead of the loop's end (kernels_spec.h): a SHADOW slot behind the last one (contexts of one small
  // window), workers on a stream of their own (lowest priority: a third pool of hardware queues), one graph of SIDE_ROUNDS rounds
  // per marginalization flag and hand-over variant.  MAIL_TICKET: the ticket of the call in flight, echoed into MAIL_ECHO by the worker
  // that delivers its prior.
  bool shadow = false;          // the blob has batch + WORKERS slots, the last ones the shadows of slot 0
  bool marg_ahead = true;       // debug (lfvio_debug_configure): off = every call ends with the serial tail
  hipGraphExec_t side[WORKERS][2][2] = {};  // [worker][marg_flag][publish]
  long long stat_ahead_calls = 0, stat_ahead_hits = 0;  // calls with workers | priors a worker delivered
  bool stage_busy = false;  // stage_event is recorded and not yet waited for
  double up_us[4] = {0, 0, 0, 0};  // last upload: host packing | collecting the chained prior | prior + copies enqueued | final synchronization (lfvio_debug_query "upload_times")
  // a prior collected on the caller's behalf because the slots had to be re-allocated while its call was in flight
  // (reserve, CallState::HELD): lfvio_batch_optimize_finish / lfvio_batch_upload_chained hand it over
  std::unique_ptr<LfvioPrior> held;
  int mail_seq = 0;             // sequence number of the last upload (Slot::mail_seq)
  std::unique_ptr<LfvioPrior> chain_struct;  // the structure-only prior of a device-chained upload
  // lfvio_solve_relo (relo.inc): the route's device blob and pinned staging blob, the loop's `done` word read per pass
  DevBuf<char> d_relo;
  PinBuf<char> h_relo;
  int relo_done_word = 0;
  bool relo_force = false;  // lfvio_debug_configure "relo_route": the relo route even without a match
  bool debug_break_chain = false;  // lfvio_debug_configure "break_next_chain": the next device-chained upload promises a prior of another size than the device will find
  bool use_graph = true;
  int stat_chunks = 0;  // graph launches of the last synchronous solve loop (debug)
  int last_passes = 0;  // passes of the trust-region loop the last synchronous call used (slowest slot)
  int last_iters = 0;   // ... and, for one window, the iterations they covered: a window whose steps are mostly rejected gets more speculative candidates per pass
  bool fixed_spec = false;  // lfvio_debug_configure "spec_count": a fixed number of candidates (measurements)
  int spec_count = 3;   // candidates per pass of a speculating launch: radius, radius / 2, radius / 4 (, radius / 8)
  DevBuf<int> d_lwt;  // static table of k_linw's phase 3 (kernels_linw.h LWT_*)
  DevBuf<int> d_asm;  // static scatter table of k_solve_dense<true> (kernels_solve.h ASM_*)
  bool shard_group = false;  // the resident shard is driven by an lfvio_group (two collectives per pass: shard.inc phase 4)
  int shard_kmax0 = -1;  // lfvio_shard_begin: the longest track among the WHOLE window's frame-0 landmarks (0: none), for the marginalization's plan
  int lm_half = 1;       // windows of at most SPEC_MAX_LM landmarks: 8 lanes per track in k_lin's landmark role (lfvio_debug_configure "lm_half" 0: the 4-lane form)
  int linw_mode = 1;     // 1: resident batches linearize with k_linw when every slot of the launch carries a plan; 0: never (k_lin roles + k_sum);
                         // 2: any launch of planned windows, however few (tests).  lfvio_debug_configure "linw"
  double init_radius = 1e4;  // initial_trust_region_radius of the windows uploaded from now on (lfvio_debug_configure "initial_radius")
  double fn_tol = 1e-6;  // function_tolerance of the windows uploaded from now on (lfvio_debug_configure "function_tolerance")
  bool force_eig = false;  // debug: k_marg_solve takes the eigen-decomposition path for the dropped block even when the Cholesky path applies
  // landmark-sharded mode (multi-GPU)
  bool shard_active = false;
  int shard_begin = 0, shard_end = 0, shard_state = 0;
  std::vector<int> sh_start, sh_off;
  // stream-ordered sharded driver: ring of pinned flag records, one per enqueued decision (shard.inc)
  PinBuf<int> h_flags;
  long long flag_head = 0, flag_tail = 0;
};

namespace {

int out_of_memory(lfvio_ctx *c, const char *what) {  // a Buf that could not grow, under the text its call site has always reported
  c->err = what;
  return LFVIO_ERR_DEVICE;
}
// keep_side: the workers' graphs (kernels_spec.h) stay — they are captured for the slot's CAPACITY, not for the resident window's launch
// dimensions, and a stream of windows changes those every few frames
void destroy_graph(lfvio_ctx *c, bool keep_side = false) {
  // (a graph whose tail is still running behind an early state is not destroyed under it)
  if (c->stream && c->call.graphs_dropped()) (void)hipStreamSynchronize(c->stream);
  if (c->graph) {
    (void)hipGraphExecDestroy(c->graph);
    c->graph = nullptr;
  }
  if (!keep_side) {
    for (auto &st : c->sstream)
      if (st) (void)hipStreamSynchronize(st);  // (rounds that found nothing to do may still be draining)
    for (auto &wk : c->side)
      for (auto &row : wk)
        for (auto &t : row)
          if (t) (void)hipGraphExecDestroy(t), t = nullptr;
  }
  for (auto &t : c->chunk)
    if (t) (void)hipGraphExecDestroy(t), t = nullptr;
  for (auto &row : c->tail)
    for (auto &t : row)
      if (t) (void)hipGraphExecDestroy(t), t = nullptr;
  for (auto &var : c->first)
    for (auto &plane : var)
      for (auto &row : plane)
        for (auto &t : row)
          if (t) (void)hipGraphExecDestroy(t), t = nullptr;
}

// The first graph of the next call is sized from the calls before it.  A pass the window does not need returns at once (~15 us of
// launches for the four kernels); a pass it needs and the graph does not carry is a round trip to the host and another graph
// launch (~60 us).  A resident window re-solved again and again needs the same number every time; the windows of a stream vary by
// one or two passes from frame to frame (4 .. 8 on the synthetic stream): the most any of the last four calls needed covers nearly
// all of them (measured on the stream: 0.881 ms per window with the last call's count, 0.862 with a fixed 8).
void predict(lfvio_ctx *c) {
  c->recent_passes[c->recent_head++ & 3] = c->last_passes;
  int m = 1;
  for (int k = 0; k < 4; k++) m = std::max(m, c->recent_passes[k]);
  c->predict_passes = m;
}
// The counts of a call whose loop has ended (lfvio_debug_query "last_call"); act & FEED_PREDICTION: ... for the first time, so they
// size the next call's first graph
void record_call(lfvio_ctx *c, int passes, int iters, unsigned act) {
  c->last_passes = std::max(passes, 1), c->last_iters = iters;
  if (act & CallState::FEED_PREDICTION) predict(c);
}
volatile int *mail_word(lfvio_ctx *c, MailWord w) { return (volatile int *)c->h_mail.get() + w; }
// The call whose loop has just ended on stream 0 left its prior to a worker on the second stream (TAIL_WORKER, kernels_spec.h): wait
// for the worker's echo of the call's ticket — it follows the prior's arrival in slot 0 (and in the mailbox) behind a system-scope
// fence.  Stream 0 is idle when this is called.
int wait_side(lfvio_ctx *c) {
  const CallState::Workers w = c->call.take_workers();
  if (w == CallState::NO_WORKERS) return LFVIO_OK;
  int ts = 0;
  if (w == CallState::KNOWN) ts = c->h_pending->tail_state;
  else HIPCHK(c, hipMemcpy(&ts, c->d_base + offsetof(Slot, tail_state), sizeof ts, hipMemcpyDeviceToHost));  // (a tail graph of its own: rare)
  const int *echo = (const int *)mail_word(c, MAIL_ECHO);
  if (ts == TAIL_WORKER) {
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(echo, __ATOMIC_ACQUIRE) != c->call.ticket) {
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) {
        c->call.worker_wait_timed_out();
        c->err = "the marginalization handed to a worker stream did not arrive";
        return LFVIO_ERR_DEVICE;
      }
    }
  }
  if (__atomic_load_n(echo, __ATOMIC_ACQUIRE) == c->call.ticket) c->stat_ahead_hits++;
  *mail_word(c, MAIL_TICKET) = 0;  // (whatever runs k_setup on this slot next without workers of its own — a standalone marginalization, a debug sweep — publishes nothing)
  return LFVIO_OK;
}
constexpr const char *CHAIN_ERR_TEXT = "the prior this window was to take over on the device was not there (the marginalization before it produced none): it ran without a prior";
// The tail of a call whose solution went out early (lfvio_batch_optimize_begin) is still on the stream: wait for it and
// take the bookkeeping its graph left in the pinned block.  First statement of everything that touches the slots.
// OVERTAKE_PIPELINED (lfvio_batch_optimize_begin only): a window uploaded behind a marginalization that is still running
// (lfvio_batch_upload_chained_device) is optimized behind it too — everything is ordered by the stream, nothing is waited for.
// (the chain error of the call in flight is not looked at here: its begin() has reported it with the state, and once is enough)
int join_inflight(lfvio_ctx *c, CallState::Overtake overtake = CallState::WAIT) {
  const unsigned act = c->call.join(overtake);
  if (!(act & CallState::DRAIN)) return LFVIO_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const bool handed = c->h_pending && c->call.handed_to_worker(c->h_pending->tail_state == TAIL_WORKER);  // the prior was a worker's (kernels_spec.h)
  if (int rc = wait_side(c)) return rc;
  if (act & CallState::READ_FIRST_WORDS) {
    record_call(c, c->h_pending->passes_used, c->h_pending->iters_done, act);
    if (c->h_pending->tail_state != TAIL_DONE && !handed) {
      c->err = "the marginalization behind an early solution did not finish";
      return LFVIO_ERR_DEVICE;
    }
  }
  return LFVIO_OK;
}

// After a graph launch: the first of "the solution is in the mailbox" (true) and "everything enqueued has run" (false: the
// window was not done within these passes and the gated gauge fix did not run, or there is no mailbox for this window).
// (the flag is the sequence number of the resident window's upload: a window optimized behind the marginalization of the one
// before must not take that one's late prior flag for its own)
bool wait_early(lfvio_ctx *c) {
  int *flag = (int *)c->h_mail.get() + MAIL_STATE_FLAG;
  const int want = c->info[0].mail_seq;
  for (;;) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) return true;
    if (hipStreamQuery(c->stream) != hipErrorNotReady) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == want;
  }
}

constexpr int SHADOW_MAX_LM = 1024;  // capacity (with reserve()'s headroom) up to which a one-window context carries a shadow slot
int reserve(lfvio_ctx *c, int batch, int maxN, int maxM) {
  if (c->d_base && batch <= c->batch && maxN <= c->L.maxN && maxM <= c->L.maxM) return LFVIO_OK;  // (the usual case: nothing to wait for)
  if (c->call.early()) {  // the slot that holds the prior of the call in flight is about to be freed: collect it first
    if (!c->held) c->held.reset(new LfvioPrior);
    if (int rc = lfvio_batch_optimize_finish(c, c->held.get())) return rc;
    c->call.prior_held();
  }
  if (int rc = join_inflight(c)) return rc;
  batch = std::max(batch, c->batch);
  maxN = std::max(maxN, c->L.maxN);
  maxM = std::max(maxM, c->L.maxM);
  destroy_graph(c);
  MEMCHK(c, c->d_base.reset(), "hipFree(c->d_base)");
  MEMCHK(c, c->h_stage.reset(), "hipHostFree(c->h_stage)");
  MEMCHK(c, c->h_down.reset(), "hipHostFree(c->h_down)");
  c->stage_busy = false;  // (hipFree above waited for the device)
  // grow with headroom so a slowly growing window does not re-allocate every frame
  Layout L = make_layout(maxN + maxN / 4 + 64, maxM + maxM / 4 + 256);
  // one small window: a shadow slot behind it for the marginalization run ahead (kernels_spec.h)
  c->shadow = batch == 1 && L.maxN <= SHADOW_MAX_LM && c->sstream[0] && c->sstream[lfvio_ctx::WORKERS - 1] && c->d_mail;
  const size_t slots = (size_t)batch + (c->shadow ? lfvio_ctx::WORKERS : 0);
  MEMCHK(c, c->d_base.reserve(L.total * slots), "hipMalloc((void **)&c->d_base, L.total * slots)");
  HIPCHK(c, hipMemsetAsync(c->d_base, 0, L.total * slots, c->stream));
  MEMCHK(c, c->h_stage.reserve(L.linw_end), "hipHostMalloc((void **)&c->h_stage, L.linw_end, hipHostMallocDefault)");
  MEMCHK(c, c->h_down.reserve(down_bytes(L.maxN)), "hipHostMalloc((void **)&c->h_down, c->h_down_bytes, hipHostMallocDefault)");
  c->L = L;
  c->batch = batch;
  c->info.assign(batch, SlotHostInfo());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LFVIO_OK;
}

// (local_size, tangent_off, plan_marg: window_pack.h)

// a prior carries n x n of its 172 x 172 Jacobian slots: copy what is there (46 KB instead of 240 KB for n = 76)
void copy_prior(LfvioPrior *dst, const LfvioPrior *src) {
  std::memcpy(dst, src, offsetof(LfvioPrior, linearized_jacobians));
  if (src->valid && src->n > 0 && src->n <= LFVIO_MAX_PRIOR_DIM) {
    std::memcpy(dst->linearized_jacobians, src->linearized_jacobians, sizeof(double) * src->n * src->n);
    std::memcpy(dst->linearized_residuals, src->linearized_residuals, sizeof(double) * src->n);
  }
}

}  // namespace
extern "C" int lfvio_batch_optimize_finish(lfvio_ctx *c, LfvioPrior *prior);
namespace {

int check_input_prior(lfvio_ctx *c, const LfvioPrior *pr) {
  if (pr && (pr->n <= 0 || pr->n > LFVIO_MAX_PRIOR_DIM || pr->num_blocks <= 0 || pr->num_blocks > LFVIO_MAX_PRIOR_BLOCKS)) {
    c->err = "malformed prior";
    return LFVIO_ERR_ARG;
  }
  if (pr) {
    // the blocks index present[kind][frame], prior_cmap and prior_inv below: refuse anything that would leave them
    for (int i = 0; i < pr->num_blocks; i++) {
      const int k = pr->blocks[i].kind, f = pr->blocks[i].frame, idx = pr->block_idx[i];
      const bool framed = k == LFVIO_BLOCK_POSE || k == LFVIO_BLOCK_SPEEDBIAS;
      if (k < LFVIO_BLOCK_POSE || k > LFVIO_BLOCK_TD || f < 0 || f >= LFVIO_NUM_FRAMES || (!framed && f != 0) || idx < 0 ||
          idx + local_size(k) > pr->n) {
        c->err = "malformed prior block (kind / frame / block_idx out of range)";
        return LFVIO_ERR_ARG;
      }
    }
  }
  return LFVIO_OK;
}

constexpr size_t LIN_SPLIT_WGS = 2048;  // launches of k_lin with more workgroups than this are issued role by role ...
constexpr int LINB_MAX_GROUPS = 500;     // ... in at most this many groups (two workgroups per CU: 512 at once, one of them the pose side's)
// A single window from this many landmarks on is linearized group by group (k_linb, kernels_linw.h).  A group is a latency of ~60 us
// however few there are; the role-by-role sweep grows with the window (measured, whole optimization(), profiles/r04/linb_times.txt:
// 20 000 landmarks 1.29 ms role by role / 1.34 by groups, 50 000: 1.58 / 1.48, 100 000: 1.94 / 1.63, 200 000: 3.17 / 2.39).
constexpr int LINB_MIN_LM = 40960;
constexpr int LIN_SPLIT_MIN_BATCH = 8;   // ... when they are a batch: ONE large window (100 000 landmarks: 64 us as one grid, 54 + 35 + 14 role by role) is better off with its roles overlapping

// The window's own sizes and arrays (lfvio_solve and the others that upload, lfvio_solve_relo); its prior is the caller's to check.
int check_window(lfvio_ctx *c, const LfvioWindow *w) {
  if (!w || w->num_landmarks < 0 || w->num_observations < 0) {
    c->err = "null window / negative sizes";
    return LFVIO_ERR_ARG;
  }
  const int N = w->num_landmarks, M = w->num_observations;
  if (N > 0 && (!w->start_frame || !w->obs_offset || !w->inv_depth || !w->obs_point || !w->obs_velocity ||
                !w->obs_cur_td || !w->obs_uv_y)) {
    c->err = "null landmark / observation arrays";
    return LFVIO_ERR_ARG;
  }
  if (N > 0 && (w->obs_offset[0] != 0 || w->obs_offset[N] != M)) {
    c->err = "obs_offset is not a CSR over num_observations";
    return LFVIO_ERR_ARG;
  }
  for (int l = 0; l < N; l++) {
    const int k = w->obs_offset[l + 1] - w->obs_offset[l], s = w->start_frame[l];
    if (k < 2 || s < 0 || s + k > LFVIO_NUM_FRAMES) {  // used_num >= 2, track inside the window
      c->err = "landmark with fewer than 2 observations or a track leaving the window";
      return LFVIO_ERR_ARG;
    }
  }
  if (w->estimate_td && !(w->row > 0.0)) {  // row_i = uv.y - ROW / 2 and TR / ROW (projection_td_factor.cpp:20-21, 54-55)
    c->err = "estimate_td needs row > 0";
    return LFVIO_ERR_ARG;
  }
  return LFVIO_OK;
}

// What an upload is asked for beyond the window and its slot.
// chain (lfvio_batch_upload_chained): the window's prior is *chain, and if a call is still in flight on the context (the
// marginalization behind an early state), it is THAT call's prior: the landmark tables and gather lists of the new window —
// nine tenths of the host work of an upload — are packed while the device finishes it, then the prior is taken from the
// mailbox into *chain and the upload goes on with it.
// device_chain (lfvio_batch_upload_chained_device): the prior of the call in flight STAYS on the device — nothing is waited for or
// collected; the new window's prior has the structure the host planned for that marginalization (SlotHostInfo::marg_out) and the
// values k_prior_chain copies out of Slot::prior_out behind these copies, which the stream puts behind the marginalization.
struct UploadMode {
  int sharded = 0;    // Slot::sharded: the slot holds a rank's share of the window (lfvio_shard_begin; 2: driven by an lfvio_group)
  int pose_side = 1;  // Slot::pose_side
  LfvioPrior *chain = nullptr;
  bool device_chain = false;
};

// The structure-only prior of a device-chained upload (lfvio_ctx::chain_struct), from what the host planned for the marginalization in flight
int device_chain_prior(lfvio_ctx *c, int slot, const UploadMode &mode) {
  if (slot != 0 || mode.sharded || !c->call.can_chain_on_device() || !c->info[0].resident) {
    c->err = "lfvio_batch_upload_chained_device: no call in flight on slot 0 (lfvio_batch_optimize_begin) whose prior could be taken over";
    return LFVIO_ERR_ARG;
  }
  const SlotHostInfo::MargOut &mo = c->info[0].marg_out[c->call.marg_flag];
  if (!mo.valid) {
    c->err = "lfvio_batch_upload_chained_device: the marginalization in flight passes its input prior through (MARGIN_SECOND_NEW without a "
             "prior on the newest pose) — use lfvio_batch_upload_chained";
    return LFVIO_ERR_ARG;
  }
  if (!c->chain_struct) c->chain_struct.reset(new LfvioPrior);
  LfvioPrior *sp = c->chain_struct.get();
  std::memset(sp, 0, offsetof(LfvioPrior, linearized_jacobians));
  sp->valid = 1, sp->n = mo.n, sp->m = mo.m, sp->num_blocks = mo.nb;
  if (c->debug_break_chain) sp->n = mo.n + 1, c->debug_break_chain = false;  // (k_prior_chain finds a prior of mo.n rows: the failure path, end to end)
  for (int i = 0; i < mo.nb; i++) sp->blocks[i].kind = mo.kind[i], sp->blocks[i].frame = mo.frame[i], sp->block_idx[i] = mo.idx[i];
  return LFVIO_OK;
}

// What pack_window (window_pack.h) takes from the context
PackOptions pack_options(const lfvio_ctx *c, int slot, const LfvioWindow *w, const UploadMode &mode) {
  const int N = w->num_landmarks;
  PackOptions o;
  o.slot = slot, o.sharded = mode.sharded, o.pose_side = mode.pose_side;
  o.mail = (long long)(uintptr_t)c->d_mail;
  o.shadow = c->shadow, o.marg_ahead = c->marg_ahead;
  o.lm_half = c->lm_half;
  o.want_linw = c->linw_mode != 0 && !mode.sharded && N <= SPEC_MAX_LM && (c->batch >= LIN_SPLIT_MIN_BATCH || c->linw_mode == 2);
  // a large single window: the same strips as groups of one start frame, one workgroup each (k_linb)
  o.want_linb = c->linw_mode != 0 && !o.want_linw && N >= (c->linw_mode == 2 ? SPEC_MAX_LM + 1 : LINB_MIN_LM);  // (a rank's share of a sharded window too)
  o.linb_max_groups = LINB_MAX_GROUPS;
  o.fn_tol = c->fn_tol, o.init_radius = c->init_radius;
  o.seq = c->mail_seq == 0x7fffffff ? 1 : c->mail_seq + 1;  // (never 0: the host clears the flags to 0)
  return o;
}

// Everything the host believes about the slot, from the staging block S and pack_window's result.  Written where the copies are
// enqueued: an upload refused on the way — or a chained one, which collects the prior of the window still resident in between —
// leaves the slot's description matching what the device holds.  From here on the device copy changes (resident = false until the
// copies are enqueued).
void commit_slot_info(lfvio_ctx *c, int slot, const LfvioWindow *w, const Slot *S, const LfvioPrior *pr, bool device_chain, const PackResult &r, int seq) {
  SlotHostInfo &info = c->info[slot];
  info.resident = false;
  info.N = r.N, info.M = r.M;
  info.prior_n = S->prior_valid ? S->prior_n : 0;
  info.max_iter = w->max_num_iterations, info.max_seconds = w->max_solver_time_in_seconds;
  info.perm.swap(c->perm_build);
  info.gLm = S->nLmBlocks, info.gLw = S->nSchurParts, info.gCh = r.nChunks, info.gSc = S->nSchurParts;
  info.has_in_prior = pr != nullptr;
  info.in_prior_device = pr && device_chain;
  if (pr && device_chain) std::memcpy(&info.in_prior, pr, offsetof(LfvioPrior, linearized_jacobians));  // (structure; the values are the device's)
  else if (pr) copy_prior(&info.in_prior, pr);
  for (int f = 0; f < 2; f++) {
    SlotHostInfo::MargOut &mo = info.marg_out[f];
    const MargPlan &mp = S->marg[f];
    mo.valid = mp.valid, mo.n = mp.n, mo.m = mp.m15 + mp.N0, mo.nb = mp.nb;
    for (int i = 0; i < mp.nb; i++) mo.kind[i] = mp.kind[i], mo.frame[i] = mp.shifted_frame[i], mo.idx[i] = mp.idx[i];
  }
  info.mail_seq = c->mail_seq = seq;
  info.spec_on = S->spec_on != 0;
  info.offs_first = r.offs_first, info.offs_all = r.offs_all;
  info.marg_n = std::max(S->marg[0].valid ? S->marg[0].n : 0, S->marg[1].valid ? S->marg[1].n : 0);
  info.linw_ok = r.linw;
  info.linb_ok = r.linb, info.linb_ng = r.linb_ng;
}

// The staging block's way to the slot
int enqueue_window_copies(lfvio_ctx *c, int slot, const LfvioPrior *pr, bool device_chain, const PackResult &r) {
  const Layout &L = c->L;
  char *h = c->h_stage, *d = c->d_base + (size_t)slot * L.total;
  // (an upload behind a call in flight whose prior a worker on the second stream may own: it reads this slot's inputs until it delivers)
  if (slot == 0 && c->call.workers_outstanding()) hipLaunchKernelGGL(k_spec_wait, dim3(1), dim3(64), 0, c->stream, d);
  // header prefix + input arrays (two copies: the work-pointer part of the header is written once, put_work_pointers)
  HIPCHK(c, hipMemcpyAsync(d, h, offsetof(Slot, x), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + L.in_begin, h + L.in_begin, (r.lists_cached ? L.sum_off : L.sum_items + (size_t)r.used_items * 4) - L.in_begin, hipMemcpyHostToDevice,
                           c->stream));
  if (pr && !device_chain) HIPCHK(c, hipMemcpyAsync(d + L.prior_J, h + L.prior_J, sizeof(double) * pr->n * pr->n, hipMemcpyHostToDevice, c->stream));
  if (device_chain) {
    hipLaunchKernelGGL(k_prior_chain, dim3(1, 1), dim3(256), 0, c->stream, d, L.total);  // (the slot's own blob as base)
    // the call that was in flight is now only work on the stream in front of this window's: nothing of it is left to collect
    c->call.chained_on_device();
  }
  if (r.linw) HIPCHK(c, hipMemcpyAsync(d + L.linw_begin, h + L.linw_begin, L.pm_pair + (size_t)std::max(r.M - r.N, 0) - L.linw_begin, hipMemcpyHostToDevice, c->stream));
  if (r.linb) HIPCHK(c, hipMemcpyAsync(d + L.linb_lm0, h + L.linb_lm0, L.linw_end - L.linb_lm0, hipMemcpyHostToDevice, c->stream));
  return LFVIO_OK;
}

// The pointer members of Slot that lead to its work arrays, all but prior_A: fixed per slot until the next reserve()
#define SLOT_WORK_POINTERS(X)                                                                                                     \
  X(lam) X(lamE) X(cost_partE)                                                                                                    \
  X(a) X(b) X(W) X(Wt) X(scale_l) X(grad_l) X(gn_l) X(diag_l) X(einv_l) X(d1) X(d2)                                                \
  X(gram_part) X(pairG) X(schur_part) X(schur_sum) X(xch) X(gp) X(lm_part) X(cost_part) X(imu_out) X(imu_raw)                      \
  X(Hpp) X(mscr) X(eig_aux)

// Written once per slot, and with slot 0 of a context that keeps them into its shadow slots: a shadow's work arrays are its own, laid
// out like every slot's (the members are self-relative: the same bytes) — but J0^T J0 of the input prior, which k_setup forms once
// per call, is read from slot 0: a shadow's prior_A leads back there.
int put_work_pointers(lfvio_ctx *c, int slot) {
  const Layout &L = c->L;
  Slot W;
  std::memset(&W, 0, sizeof W);
  W.lam[0].set(&W, L.lam[0]), W.lam[1].set(&W, L.lam[1]);
  for (int k = 0; k < SPEC_EXTRA; k++) W.lamE[k].set(&W, L.lamE[k]);
  W.cost_partE.set(&W, L.cost_partE);
  W.prior_A.set(&W, L.prior_A);
  W.a.set(&W, L.a), W.b.set(&W, L.b), W.W.set(&W, L.W), W.Wt.set(&W, L.Wt);
  W.scale_l.set(&W, L.scale_l), W.grad_l.set(&W, L.grad_l), W.gn_l.set(&W, L.gn_l);
  W.diag_l.set(&W, L.diag_l), W.einv_l.set(&W, L.einv_l), W.d1.set(&W, L.d1), W.d2.set(&W, L.d2);
  W.gram_part.set(&W, L.gram_part), W.pairG.set(&W, L.pairG);
  W.schur_part.set(&W, L.schur_part);
  W.xch.set(&W, L.xch);
  W.schur_sum.set(&W, L.xch + (size_t)XOFF_S * 8), W.gp.set(&W, L.xch + (size_t)XOFF_G * 8), W.Hpp.set(&W, L.xch + (size_t)XOFF_H * 8);
  W.lm_part.set(&W, L.lm_part), W.cost_part.set(&W, L.cost_part), W.imu_out.set(&W, L.imu_out), W.imu_raw.set(&W, L.imu_raw);
  W.mscr.set(&W, L.mscr);
  W.eig_aux.set(&W, L.eig_aux);
  const int shadows = (c->shadow && slot == 0) ? lfvio_ctx::WORKERS : 0;
  GP<double> prior_A[1 + lfvio_ctx::WORKERS];
  for (int k = 0; k <= shadows; k++) {
    const size_t target = k == 0 ? (size_t)slot : (size_t)(c->batch + k - 1);
    char *ds = c->d_base + target * L.total;
    // field by field so that only pointer members are touched
#define PUT(field) HIPCHK(c, hipMemcpyAsync(ds + offsetof(Slot, field), &W.field, sizeof W.field, hipMemcpyHostToDevice, c->stream));
    SLOT_WORK_POINTERS(PUT)
#undef PUT
    prior_A[k].off = W.prior_A.off - (long long)((target - (size_t)slot) * L.total);
    HIPCHK(c, hipMemcpyAsync(ds + offsetof(Slot, prior_A), &prior_A[k], sizeof prior_A[k], hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // W is on the stack
  return LFVIO_OK;
}
#undef SLOT_WORK_POINTERS

// Pack one window into the pinned staging block (window_pack.h) and upload it to slot `slot`.
int upload_window(lfvio_ctx *c, int slot, const LfvioWindow *w, const UploadMode &mode = UploadMode()) {
  const bool device_chain = mode.device_chain;
  LfvioPrior *chain = mode.chain;
  if (device_chain) {
    if (int rc = device_chain_prior(c, slot, mode)) return rc;
    chain = c->chain_struct.get();
  }
  const bool chained = !device_chain && chain && c->call.pending() && slot == 0;
  const auto t_up0 = std::chrono::steady_clock::now();
  auto lap = [&](int k, std::chrono::steady_clock::time_point from) {
    const auto now = std::chrono::steady_clock::now();
    c->up_us[k] = std::chrono::duration<double>(now - from).count() * 1e6;
    return now;
  };
  if (!chained && !device_chain)
    if (int rc = join_inflight(c)) return rc;
  if (int rc = check_window(c, w)) return rc;
  const LfvioPrior *given = chain ? chain : w->prior;
  const LfvioPrior *pr = (given && given->valid) ? given : nullptr;  // (chained: not known before the call in flight has finished)
  if (!chained)
    if (int rc = check_input_prior(c, pr)) return rc;
  const Layout &L = c->L;
  char *h = c->h_stage;
  if (c->stage_busy) {  // the previous upload's copies out of the staging block (long done, unless uploads come back to back)
    c->stage_busy = false;
    HIPCHK(c, hipEventSynchronize(c->stage_event));
  }
  SlotHostInfo &info = c->info[slot];
  const PackOptions opt = pack_options(c, slot, w, mode);
  PackResult r;
  if (const char *text = pack_window(w, L, h, opt, c->perm_build, info.list_key, info.list_items, info.uploaded, &r)) {
    c->err = text;
    return LFVIO_ERR_ARG;
  }
  auto t_up1 = lap(0, t_up0);
  c->up_us[1] = 0.0;
  if (chained) {
    // everything above was host work on the staging block; the prior of the call in flight is needed from here on
    // (c->info[0] still describes THAT window's prior: marg_n, the input prior a pass-through hands back)
    if (int rc = lfvio_batch_optimize_finish(c, chain)) return rc;
    pr = chain->valid ? chain : nullptr;
    if (int rc = check_input_prior(c, pr)) return rc;
    t_up1 = lap(1, t_up1);
  }
  if (const char *text = pack_prior(w, pr, device_chain, L, h, r, mode.sharded, c->shard_kmax0)) {
    c->err = text;
    return LFVIO_ERR_ARG;
  }
  commit_slot_info(c, slot, w, (const Slot *)h, pr, device_chain, r, opt.seq);
  if (int rc = enqueue_window_copies(c, slot, pr, device_chain, r)) return rc;
  info.list_items = r.used_items;  // (only now: an upload refused half-way leaves the key without lists on the device)
  if (!info.uploaded) {
    if (int rc = put_work_pointers(c, slot)) return rc;
    info.uploaded = true;
  }
  if (r.linb)  // (the slot's own blob as base)
    hipLaunchKernelGGL(k_linb_gather, dim3((std::max(r.N, r.M - r.N) + 255) / 256, 1), dim3(256), 0, c->stream, c->d_base + (size_t)slot * L.total, L.total);
  // The staging block is reused by the next upload: that one waits for these copies (an event), this one does not — what
  // follows an upload is an optimization on the same stream, and a round trip to the device saved here is ~30 us of the call.
  const auto t_up2 = lap(2, t_up1);
  if (!c->stage_event) HIPCHK(c, hipEventCreateWithFlags(&c->stage_event, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->stage_event, c->stream));
  c->stage_busy = true;
  lap(3, t_up2);
  info.resident = true;
  return LFVIO_OK;
}

// A HIPCHK that returns in the middle of a stream capture would leave the stream capturing (every later call on it fails):
// the guard ends the capture and drops the partial graph on any early return.
struct CaptureGuard {
  hipStream_t stream;
  bool active = true;
  explicit CaptureGuard(hipStream_t s) : stream(s) {}
  hipError_t end(hipGraph_t *g) {
    active = false;
    return hipStreamEndCapture(stream, g);
  }
  ~CaptureGuard() {
    if (!active) return;
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(stream, &g);
    if (g) (void)hipGraphDestroy(g);
  }
};

// What enqueue() puts on `stream`, captured and instantiated as *out; an error enqueue() returns drops the partial graph
template <class F>
int capture_graph(lfvio_ctx *c, hipStream_t stream, hipGraphExec_t *out, F &&enqueue) {
  hipGraph_t graph;
  HIPCHK(c, hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  CaptureGuard guard(stream);
  if (int rc = enqueue()) return rc;
  HIPCHK(c, guard.end(&graph));
  HIPCHK(c, hipGraphInstantiate(out, graph, nullptr, nullptr, 0));
  HIPCHK(c, hipGraphDestroy(graph));
  return LFVIO_OK;
}

constexpr int CH_BUCKET = 16;

Grid grid_for(lfvio_ctx *c, int count) {
  Grid g{1, 1, 1, 1, 1};
  for (int s = 0; s < count; s++) {
    g.ch_raw = std::max(g.ch_raw, c->info[s].gCh);
    g.lm = std::max(g.lm, c->info[s].gLm);
    g.lw = std::max(g.lw, c->info[s].gLw);
    g.ch = std::max(g.ch, c->info[s].gCh);
    g.sc = std::max(g.sc, c->info[s].gSc);
  }
  // The launch dimensions are the key of the captured graphs, and in a stream of windows from one estimator the number of
  // frame-pair chunks changes with almost every frame: round it up to whole groups of four workgroups (a workgroup of
  // k_lin takes four chunks) so that neighbouring windows share a graph.  Every kernel tests its block index against
  // the slot's own counts (the grid of a resident batch is the maximum over its slots anyway), so spare blocks return.
  g.ch = (g.ch + CH_BUCKET - 1) / CH_BUCKET * CH_BUCKET;
  return g;
}

// what the sweeps of slots [0, count) need: bit 0 the sweep at the uploaded state, bit 1 every sweep
int slots_offs(const lfvio_ctx *c, int count) {
  int r = 0;
  for (int k = 0; k < count; k++) r |= (c->info[k].offs_first ? 1 : 0) | (c->info[k].offs_all ? 2 : 0);
  return r;
}

SetupLaunch setup_launch(lfvio_ctx *c, int count, int lm, bool zero_wt) {
  bool compact = count >= 8;
  for (int s = 0; compact && s < count; s++) compact = c->info[s].prior_n <= SETUP_TILED_MAXN;
  return {(compact ? 3 : SETUP_WGS) + (lm + 3) / 4, (zero_wt ? 1 : 0) | (compact ? 4 : 0)};
}

// How a launch in `mode` over slots [0, count) linearizes:
//  - k_linw, window by window (kernels_linw.h): a resident batch whose windows all carry a LinwPlan, in the solve passes and the
//    marginalization's sweep behind them (linw_mode 2: however few windows);
//  - k_linb + k_sumb, group by group: large single windows that carry a group list, in the solve passes only (the marginalization's
//    sweep of such a window stays with the roles: one launch per call), and a rank's share of a sharded window under the same
//    condition (either way its sums land in the exchange buffer);
//  - k_lin role by role + k_sum otherwise; a resident batch sends the roles out as separate launches (`split`, and without the
//    transposed copy of W: its k_dogleg reads the compact rows).
Route route_for(lfvio_ctx *c, int count, int mode) {
  Route r;
  r.count = count;
  r.g = grid_for(c, count);
  r.role_wgs = (size_t)count * (r.g.lw + (r.g.ch + 3) / 4 + LFVIO_WINDOW_SIZE + 1);
  r.split = count >= LIN_SPLIT_MIN_BATCH && r.role_wgs > LIN_SPLIT_WGS;
  bool linw = true, linb = count > 0;
  int ng = 0;
  for (int s = 0; s < count; s++) {
    linw = linw && c->info[s].linw_ok, linb = linb && c->info[s].linb_ok;
    ng = std::max(ng, c->info[s].linb_ng);
  }
  const bool solve = mode == MODE_SOLVE;
  const bool marg_sweep = (mode & (MODE_GATED - 1)) >= MODE_MARG && !(mode & (MODE_DECIDE | MODE_NOCOUNT));
  if (c->linw_mode != 0 && !c->shard_active && linw && (solve || marg_sweep) && (c->linw_mode == 2 || r.split)) r.sweep = Route::LINW;
  else if (c->linw_mode != 0 && solve && linb && (!c->shard_active || count == 1)) r.sweep = Route::LINB;
  else r.sweep = Route::ROLES;
  // (grid of k_linb: the groups of the largest resident window and the pose side's workgroup, rounded up so that a captured graph
  // serves the next window of about that size too — a workgroup past a slot's own count returns at once; part of the graphs' key)
  r.linb_gx = r.sweep == Route::LINB ? (ng + 1 + 63) / 64 * 64 : 0;
  r.setup = setup_launch(c, count, r.g.lm, r.sweep == Route::LINW);
  r.offs = slots_offs(c, count);
  return r;
}

// spec: the speculation variant; passes: of a graph that carries a fixed number; with_setup: the graph carries k_setup
GraphKey graph_key(const Route &r, int spec, int passes, bool with_setup) {
  GraphKey k;
  k.count = r.count, k.lm = r.g.lm, k.ch = r.g.ch, k.sc = r.g.sc, k.sweep = r.sweep, k.linb_gx = r.linb_gx, k.offs = r.offs;
  k.setup = with_setup ? r.setup.bits : 0, k.spec = spec, k.passes = passes;
  return k;
}

void launch_setup(lfvio_ctx *c, const Route &r, int mode) {
  hipLaunchKernelGGL(k_setup, dim3(r.setup.gx, r.count), dim3(256), 0, c->stream, c->d_base, c->L.total, mode, r.setup.bits);
}

// offs: the visual sweep in the instantiation that knows the off-sphere flavour (k_lin, kernels_lin.h) — launch(std::true_type) —
// or in the one that does not; the loop's launches say what they need (slots_offs), the one-off sweeps take the one that is always right
template <class F>
void with_offs(bool offs, F &&launch) {
  if (offs) launch(std::true_type());
  else launch(std::false_type());
}

void launch_lin(lfvio_ctx *c, const Route &r, int mode, bool offs) {
  const int count = r.count, lw = r.g.lw, gram_wgs = (r.g.ch + 3) / 4;  // one chunk per wave
  const size_t st = c->L.total;
  const SlotArgs sa = slot_args(c->L);  // (baked into a captured graph like SumArgs: whatever changes the Layout — reserve() — drops the graphs)
  with_offs(offs, [&](auto o) {
    if (!r.split) {
      hipLaunchKernelGGL((k_lin<LIN_ROLE_ALL, decltype(o)::value>), dim3(lw + gram_wgs + LFVIO_WINDOW_SIZE + 1, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st,
                         mode, lw, gram_wgs, sa);
      return;
    }
    // A resident batch: the roles go out as separate launches, each of a kernel compiled for that role alone.  Measured at 512 windows of 300 landmarks:
    // landmark role 115 us + Gram role 175 us + IMU / prior roles 104 us on their own, 679 us as ONE grid — workgroups of four
    // different code paths side by side on every CU (the sweep is ~30 KB of straight-line code per role) do not share an
    // instruction cache well; two more launches cost 9 us.
    hipLaunchKernelGGL((k_lin<LIN_ROLE_LM, decltype(o)::value>), dim3(lw, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st, mode, lw, 0, sa);
    hipLaunchKernelGGL((k_lin<LIN_ROLE_GRAM, decltype(o)::value>), dim3(gram_wgs, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st, mode | MODE_NOCOUNT, 0, gram_wgs, sa);
  });
  if (!r.split) return;
  const bool raw = (mode & (MODE_GATED - 1)) == MODE_SOLVE && !(mode & (MODE_GATED | MODE_DECIDE));
  if (raw) hipLaunchKernelGGL(k_imu_raw, dim3((count * LFVIO_WINDOW_SIZE + 63) / 64), dim3(64), 0, c->stream, c->d_base, st, count);
  if (raw) hipLaunchKernelGGL((k_lin<LIN_ROLE_POSE_RAW, false>), dim3(LFVIO_WINDOW_SIZE + 1, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st, mode | MODE_NOCOUNT, 0, 0, sa);
  else hipLaunchKernelGGL((k_lin<LIN_ROLE_POSE, false>), dim3(LFVIO_WINDOW_SIZE + 1, count), dim3(LIN_THREADS), 0, c->stream, c->d_base, st, mode | MODE_NOCOUNT, 0, 0, sa);
}

// fixed-order reduction of the partials; two levels once a single k_sum thread would have to walk hundreds of them
void launch_sum(lfvio_ctx *c, const Route &r, int mode) {
  const int count = r.count;
  const Grid &g = r.g;
  const size_t st = c->L.total;
  // (from the unrounded chunk count: a slot has pre_gram set iff ITS count exceeds the limit — with the rounded one a window
  // of 241 or 242 chunks launched k_presum for gather lists that do not use its output)
  const int pre = (g.ch_raw > PRE_CHUNK_LIMIT || g.sc > 4 * PRE_GROUP) ? 1 : 0;
  const int groups = (g.sc + PRE_GROUP - 1) / PRE_GROUP;
  if (pre) hipLaunchKernelGGL(k_presum, dim3(NPAIR + (SCHUR_LEN / 256) * groups + 1, count), dim3(256), 0, c->stream, c->d_base, st, mode, groups);
  const Layout &L = c->L;
  const SumArgs sa{(long long)L.sum_off, (long long)L.sum_end_marg, (long long)L.sum_items, (long long)L.gram_part, (long long)L.pairG, (long long)L.imu_out,
                   (long long)L.prior_A};
  hipLaunchKernelGGL(k_sum, dim3(HPP_BLOCKS + SCHUR_LEN / 256 + 1, count), dim3(256), 0, c->stream, c->d_base, st, mode, pre, sa);
}

LinwArgs linw_args(const lfvio_ctx *c) {
  const Layout &L = c->L;
  LinwArgs a;
  a.anc0 = (long long)L.anc[0], a.anc_stride = (long long)(L.anc[1] - L.anc[0]);
  a.pmo0 = (long long)L.pmo[0], a.pmo_stride = (long long)(L.pmo[1] - L.pmo[0]);
  a.Wt = (long long)L.Wt, a.lam[0] = (long long)L.lam[0], a.lam[1] = (long long)L.lam[1];
  a.a = (long long)L.a, a.b = (long long)L.b, a.scale_l = (long long)L.scale_l, a.diag_l = (long long)L.diag_l, a.grad_l = (long long)L.grad_l;
  a.einv_l = (long long)L.einv_l, a.imu_out = (long long)L.imu_out;
  a.Hpp = (long long)(L.xch + (size_t)XOFF_H * 8), a.gp = (long long)(L.xch + (size_t)XOFF_G * 8), a.schur_sum = (long long)(L.xch + (size_t)XOFF_S * 8);
  a.part = (long long)L.schur_part, a.wt_ld = L.capLmBlocks * LM_BLOCK;
  a.asm_tab = c->d_lwt;
  return a;
}

// One linearization of the route's slots.  decide: the trust-region bookkeeping of the pass before rides in k_lin's prologue
void launch_sweep(lfvio_ctx *c, const Route &r, int mode, bool offs, bool decide = false) {
  if (r.sweep == Route::ROLES) {
    launch_lin(c, r, mode | (decide ? MODE_DECIDE : 0), offs);
    launch_sum(c, r, mode);
    return;
  }
  const size_t st = c->L.total;
  with_offs(offs, [&](auto o) {
    if (r.sweep == Route::LINW)  // the window-resident sweep: one workgroup per window — pose-side factors, visual sweep, Schur; it counts the pass
      hipLaunchKernelGGL(k_linw<decltype(o)::value>, dim3(1, r.count), dim3(LW_THREADS), LW_LDS_BYTES, c->stream, c->d_base, st, linw_args(c), mode);
    else
      hipLaunchKernelGGL(k_linb<decltype(o)::value>, dim3(r.linb_gx, r.count), dim3(LW_THREADS), LW_LDS_BYTES, c->stream, c->d_base, st, linw_args(c));
  });
  if (r.sweep == Route::LINB) hipLaunchKernelGGL(k_sumb, dim3(LINB_SUM_GRID, r.count), dim3(LINB_SUM_THREADS), 0, c->stream, c->d_base, st, linw_args(c));
}

// lw: the pass was linearized by k_linw — H_pp holds the visual terms of its camera part only, the solve adds the rest on load
void launch_solve(lfvio_ctx *c, int count, bool lw = false) {
  const size_t st = c->L.total;
  const long long xo = (long long)c->L.xch, io = (long long)c->L.imu_out, po = (long long)c->L.prior_A;
  if (lw)
    hipLaunchKernelGGL(k_solve_dense<true>, dim3(1, count), dim3(SOLVE_THREADS), SOLVE_LDS, c->stream, c->d_base, st, xo, io, po, (const int *)c->d_asm);
  else
    hipLaunchKernelGGL(k_solve_dense<false>, dim3(1, count), dim3(SOLVE_THREADS), SOLVE_LDS, c->stream, c->d_base, st, xo, io, po, (const int *)nullptr);
}

// One pass of the loop (or the sweep of a marginalization), where it stands in the sequence being issued and what rides with it
struct Pass {
  bool speculate = false;          // small windows evaluate the steps for radius, radius / 2, radius / 4 in every pass (dev_types.h, SPEC_EXTRA)
  // position of the pass in the sequence (a graph, or a plain run of passes).  For small windows
  // the trust-region bookkeeping of a pass rides in the prologue of the NEXT pass's k_lin (MODE_DECIDE, one launch less per
  // pass); k_decide itself is only launched behind the last pass, so that the header is final where the sequence ends.
  bool first = true, last = true;
  bool gauge = false;              // the gated gauge fix follows this (last) pass: launch_iteration returns true if it went out with the bookkeeping (k_decide_gauge)
  bool publish = false;            // ... and hands the state over early (CallPlan::publish)
  bool offs = true;                // see with_offs
};
// The bookkeeping of a pass of the loop rides in the prologue of the next pass's k_lin
// (latency of few windows only: in a resident batch every workgroup of k_lin repeating the decision costs more of the
// GPU than the launch it saves)
static bool pass_merges(const Route &r) { return r.sweep != Route::LINW && r.g.lm <= DOGLEG_INLINE_BLOCKS && r.role_wgs <= LIN_SPLIT_WGS; }

// The step half of a pass behind its dense solve: landmark back-substitution, dogleg, candidates, their cost at every factor and — where it
// does not ride in the next pass's k_lin (merge) — the bookkeeping.  spec_count: candidates a speculating pass prepares.  before_decide() is
// called in front of a bookkeeping kernel of its own (not k_stepw, which carries it): nothing for the loop; lfvio_debug_step_io joins the
// stream there and copies what the bookkeeping is about to read.  Returns true if the gated gauge fix went out with the bookkeeping.
template <class F>
bool launch_step_half(lfvio_ctx *c, const Route &r, const Pass &ps, bool merge, int spec_count, F &&before_decide) {
  const int count = r.count;
  const Grid &g = r.g;
  const size_t st = c->L.total;
  const bool lw = r.sweep == Route::LINW, lb = r.sweep == Route::LINB;
  // small windows: the landmark back-substitution rides inside k_dogleg (one launch less per pass)
  const bool inl = g.lm <= DOGLEG_INLINE_BLOCKS;
  const int spec = ps.speculate && inl ? spec_count : 1;
  const int nb = g.lm + LFVIO_WINDOW_SIZE + 1;
  // few small windows: the step and the cost of its candidates in one launch (k_step)
  const bool split = r.split || lw;
  const bool fuse = inl && !split && !c->shard_active && (size_t)count * nb <= 2048;
  // a resident batch on the window-resident path: step, candidate cost and bookkeeping as ONE launch, one workgroup per window
  const bool stepw = lw && inl && spec == 1;
  if (stepw) {
    hipLaunchKernelGGL(k_stepw, dim3(1, count), dim3(STEPW_LAUNCH_THREADS), 0, c->stream, c->d_base, st);
    return false;
  }
  if (!inl && lb) hipLaunchKernelGGL(k_backsub_wt, dim3(g.lm, count), dim3(64), 0, c->stream, c->d_base, st, c->L.capLmBlocks * LM_BLOCK);
  else if (!inl) hipLaunchKernelGGL(k_backsub, dim3(g.lm, count), dim3(64), 0, c->stream, c->d_base, st);
  if (fuse) hipLaunchKernelGGL(k_step, dim3(spec * nb, count), dim3(DOGLEG_INLINE_THREADS), 0, c->stream, c->d_base, st, g.lm, spec);
  else {
    if (inl && (!split || lw)) hipLaunchKernelGGL((k_dogleg<true, true>), dim3(spec, count), dim3(DOGLEG_INLINE_THREADS), 0, c->stream, c->d_base, st, spec);
    else if (inl) hipLaunchKernelGGL((k_dogleg<true, false>), dim3(spec, count), dim3(DOGLEG_INLINE_THREADS), 0, c->stream, c->d_base, st, spec);
    else hipLaunchKernelGGL(k_dogleg<false>, dim3(spec, count), dim3(128), 0, c->stream, c->d_base, st, spec);
  }
  // four lanes per track while the GPU has room for the extra waves (latency of few windows), one when a batch fills it
  if (fuse) {
  } else if ((size_t)count * nb <= 2048)  // (four waves per workgroup: 8 192 waves = eight per SIMD)
    hipLaunchKernelGGL(k_cost<4>, dim3(spec * nb, count), dim3(256), 0, c->stream, c->d_base, st, g.lm, spec);
  else if (spec == 1 && !c->shard_active) {
    hipLaunchKernelGGL((k_cost<1, false>), dim3(g.lm + 1, count), dim3(64), 0, c->stream, c->d_base, st, g.lm, 1);
    hipLaunchKernelGGL(k_cost_imu, dim3((count * LFVIO_WINDOW_SIZE + 63) / 64), dim3(64), 0, c->stream, c->d_base, st, count);
  } else
    hipLaunchKernelGGL(k_cost<1>, dim3(spec * nb, count), dim3(64), 0, c->stream, c->d_base, st, g.lm, spec);
  if (merge && ps.last && ps.gauge) {
    before_decide();
    hipLaunchKernelGGL(k_decide_gauge, dim3(1, count), dim3(128), 0, c->stream, c->d_base, st, ps.publish ? 1 : 0);
    return true;
  }
  if (!merge || ps.last) {
    before_decide();
    hipLaunchKernelGGL(k_decide, dim3(1, count), dim3(64), 0, c->stream, c->d_base, st);
  }
  return false;
}

// r: route_for(c, count, mode)
bool launch_iteration(lfvio_ctx *c, const Route &r, int mode, const Pass &ps) {
  const bool solve = (mode & (MODE_GATED - 1)) == MODE_SOLVE && !(mode & MODE_GATED);
  const bool lw = r.sweep == Route::LINW;
  const bool merge = solve && pass_merges(r);
  launch_sweep(c, r, mode, ps.offs, merge && !ps.first);
  if ((mode & (MODE_GATED - 1)) == MODE_SOLVE) {
    launch_solve(c, r.count, lw);  // (k_sumb leaves the complete matrix)
    return launch_step_half(c, r, ps, merge, c->spec_count, [] {});
  }
  return false;
}

// number of slots that still need passes (tail = 0: solve not done; tail = 1: gated marginalization not finished)
// out[1]: the largest number of passes a slot has used so far (k_lin counts them)
__global__ void k_pending(char *base, size_t stride, int count, int *out, int tail) {
  int n = 0, used = 0;
  for (int s = threadIdx.x; s < count; s += 64) {
    const Slot *S = (const Slot *)(base + (size_t)s * stride);
    n += (tail ? S->tail_state == TAIL_DONE : S->tr.done != 0) ? 0 : 1;
    used = max(used, S->passes_used);
  }
  used = __reduce_max_sync(~0ull, used);
  if (threadIdx.x == 0) out[1] = used;
  n = __reduce_add_sync(~0ull, n);
  if (threadIdx.x == 0) *out = n;
}

// a slot that is still not done when the passes are used up ends as it is (NO_CONVERGENCE): the gated tail takes it then
__global__ void k_force_done(char *base, size_t stride, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < count) {
    Slot *S = (Slot *)(base + (size_t)s * stride);
    if (!S->tr.done) S->tr.done = 1;
    if (S->spec_on && S->tail_state == TAIL_OPEN) spec_closing(S);  // (the gated gauge fix follows: kernels_spec.h)
  }
}

constexpr int SOLVE_CHUNK = 2, MAX_FIRST_PASSES = 12;  // continuation chunk; longest first graph
constexpr int SIDE_ROUNDS = 4;  // rounds of the workers' graph (kernels_spec.h): accepted states a call can have a prior started for
// STANDALONE: lfvio_marginalize — k_setup and a sweep at the uploaded state; AFTER_LOOP: behind the static loop and its gauge fix;
// GATED: part of a graph of lfvio_batch_optimize*, per slot on `done` and tail_state
enum MargKind { MARG_STANDALONE, MARG_AFTER_LOOP, MARG_GATED };
int enqueue_marg(lfvio_ctx *c, const CallPlan &p, MargKind kind);

// After a graph launch that may raise the state flag: clear both flags, launch, `behind` (what has to go out right behind the graph),
// then *early = the solution is in the mailbox while the rest of the graph is still running (wait_early)
template <class F>
int launch_watched(lfvio_ctx *c, hipGraphExec_t graph, bool watch, bool *early, F &&behind) {
  if (watch) __atomic_store_n((int *)c->h_mail.get() + MAIL_PRIOR_FLAG, 0, __ATOMIC_RELAXED), __atomic_store_n((int *)c->h_mail.get() + MAIL_STATE_FLAG, 0, __ATOMIC_RELEASE);
  HIPCHK(c, hipGraphLaunch(graph, c->stream));
  if (int rc = behind()) return rc;
  *early = watch && wait_early(c);
  return LFVIO_OK;
}
// the counts the state came with (publish_solution)
void record_mailbox_call(lfvio_ctx *c, unsigned act) {
  record_call(c, *mail_word(c, MAIL_STATE_PASSES), ((const TRState *)(c->h_mail + MAIL_TR))->iteration, act);
}

// The graphs of an adaptive call's loop: `first` — k_setup, first_passes passes and, fused, the gated gauge fix + marginalization — and
// `chunk`, SOLVE_CHUNK passes for whatever is still open behind it.  Captured on first use, kept under chunk_key.
struct LoopGraphs {
  int first_passes = 0;
  hipGraphExec_t first = nullptr, chunk = nullptr;
};
int loop_graphs(lfvio_ctx *c, const Route &r, const CallPlan &p, int passes, LoopGraphs *G) {
  const int count = r.count;
  const Grid &g = r.g;
  const bool speculate = (size_t)count * (g.lm + LFVIO_WINDOW_SIZE + 1) <= 512;
  // How many candidates a pass prepares follows the previous call (a stream of windows from one estimator is steady): where a
  // pass covered two iterations or more — most steps rejected: the bench window's nine iterations take four passes with three
  // candidates, three with four — the fourth candidate saves a pass; where nearly every step is accepted it would only be
  // evaluated (measured with a fixed count: 0.532 / 0.511 ms resident with 3 / 4, 0.950 / 0.963 ms on the stream).
  if (speculate && !c->fixed_spec) c->spec_count = (c->last_iters > 0 && c->last_iters >= 2 * c->last_passes) ? std::min(4, 1 + SPEC_EXTRA) : 3;
  if (!c->d_pending) {
    MEMCHK(c, c->d_pending.reserve(256), "hipMalloc((void **)&c->d_pending, 256)");
    MEMCHK(c, c->h_pending.reserve(256), "hipHostMalloc((void **)&c->h_pending, 256, hipHostMallocDefault)");
  }
  const int offs = r.offs;
  const GraphKey key = graph_key(r, (int)speculate, 0, true);
  if (!(c->chunk_key == key)) {
    destroy_graph(c, c->chunk_key.count == count && ((c->chunk_key.offs ^ offs) & 2) == 0);  // (the workers' graphs: per context, but for the fixed-extrinsic bit)
    c->chunk_key = key;
  }
  const bool fuse = p.fused;
  // The first graph carries as many passes as the previous call on this context needed (a stream of windows from one
  // estimator is steady: the bench window takes 4, windows whose steps are mostly accepted 5 to 8), then — fused —
  // the gated gauge fix + marginalization; whatever is still pending afterwards continues in chunks of SOLVE_CHUNK.
  // With a cap the first graph is still the predicted one — a cap of SOLVER_TIME = 0.04 s (the shipped default) is a few
  // hundred passes away and must not cost the call its single launch — unless the cap is so tight that the predicted
  // graph could overrun it: then no more passes than fit (at the measured time per pass), down to a chunk of SOLVE_CHUNK.
  int first_passes = std::min(std::max(c->fixed_passes > 0 ? c->fixed_passes : c->predict_passes, 1), std::min(passes, MAX_FIRST_PASSES));
  if (p.max_seconds > 0.0) first_passes = std::max(std::min(SOLVE_CHUNK, passes), std::min(first_passes, (int)std::min(p.max_seconds / c->pass_seconds, 1e6)));
  G->first_passes = first_passes;
  const int sv = speculate && c->spec_count > 3 ? 1 : 0;  // (both variants stay captured: a stream may alternate)
  hipGraphExec_t &first_graph = c->first[sv][p.publish ? 1 : 0][fuse ? 1 + p.marg_flag : 0][first_passes];
  enum Head { PASSES_ONLY, SETUP_FIRST };
  auto capture = [&](hipGraphExec_t *out, Head head, int npass, bool tail) {
    const bool setup = head == SETUP_FIRST;
    return capture_graph(c, c->stream, out, [&]() -> int {
      if (setup) launch_setup(c, r, MODE_SOLVE);
      bool gauged = false;
      // (the sweep behind k_setup linearizes at the uploaded state: the only point of a call that can hold a quaternion off the unit sphere,
      // a fixed extrinsic aside — slots_offs)
      Pass ps;
      ps.speculate = speculate, ps.gauge = tail, ps.publish = p.publish;
      for (int it = 0; it < npass; it++) {
        ps.first = it == 0, ps.last = it == npass - 1, ps.offs = (offs & 2) || (setup && it == 0 && (offs & 1));
        gauged = launch_iteration(c, r, MODE_SOLVE, ps);
      }
      if (tail) {
        if (!gauged) {
          hipLaunchKernelGGL(k_gauge, dim3(1 + (g.lm + 1) / 2, count), dim3(128), 0, c->stream, c->d_base, c->L.total, 1);
          if (p.publish) hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, c->stream, c->d_base, c->L.total);  // (k_decide_gauge does it itself)
        }
        if (int rc = enqueue_marg(c, p, MARG_GATED)) return rc;
      }
      if (tail && count == 1) {
        // one window: its {tail_state .. chain_err} are the answer — copied as they are (PendingBlock), no k_pending launch
        HIPCHK(c, hipMemcpyAsync(&c->h_pending->tail_state, c->d_base + offsetof(Slot, tail_state), 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      } else {
        hipLaunchKernelGGL(k_pending, dim3(1), dim3(64), 0, c->stream, c->d_base, c->L.total, count, c->d_pending, tail ? 1 : 0);
        HIPCHK(c, hipMemcpyAsync(&c->h_pending->open, c->d_pending, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      }
      return LFVIO_OK;
    });
  };
  if (!first_graph)
    if (int rc = capture(&first_graph, SETUP_FIRST, first_passes, fuse)) return rc;
  if (!c->chunk[sv])
    if (int rc = capture(&c->chunk[sv], PASSES_ONLY, SOLVE_CHUNK, /*tail*/ false)) return rc;
  G->first = first_graph, G->chunk = c->chunk[sv];
  return LFVIO_OK;
}

// Workers for the marginalization run ahead (kernels_spec.h): SIDE_ROUNDS rounds of [k_spec_begin, k_lin, k_sum, k_marg_solve] on the shadow
// slot, captured once per marginalization flag and hand-over variant; a round that finds nothing to do is four launches that return.
int worker_graphs(lfvio_ctx *c, const Route &r, const CallPlan &p) {
  for (int wk = 0; wk < lfvio_ctx::WORKERS; wk++) {
    hipGraphExec_t *side_graph = &c->side[wk][p.marg_flag][p.publish ? 1 : 0];
    if (*side_graph) continue;
    hipStream_t ss = c->sstream[wk];
    const size_t back = (size_t)(c->batch + wk) * c->L.total;
    char *sh = c->d_base + back;
    // launch dimensions for the largest window the merged sequence takes (spare workgroups test their index against the slot's own
    // counts and return): one capture serves every window of the context
    const Layout &L = c->L;
    const int mode = (MODE_MARG + p.marg_flag) | MODE_GATED, gram_wgs = (L.capChunks + 3) / 4, lw_cap = 2 * DOGLEG_INLINE_BLOCKS;
    // (the gather lists are inputs: the shadow's copies of those members lead back into slot 0, and so do these offsets;
    // no k_presum: that is for windows of thousands of landmarks)
    const SumArgs sa{(long long)L.sum_off - (long long)back, (long long)L.sum_end_marg - (long long)back, (long long)L.sum_items - (long long)back,
                     (long long)L.gram_part, (long long)L.pairG, (long long)L.imu_out, (long long)L.prior_A - (long long)back};
    const int rc = capture_graph(c, ss, side_graph, [&]() -> int {
      for (int rd = 0; rd < SIDE_ROUNDS; rd++) {
        hipLaunchKernelGGL(k_spec_begin, dim3(1), dim3(128), 0, ss, sh, back, slot_args(L));
        // (a re-anchored state: on the sphere but for a fixed extrinsic)
        with_offs(r.offs & 2, [&](auto o) {
          hipLaunchKernelGGL((k_lin<LIN_ROLE_ALL, decltype(o)::value>), dim3(lw_cap + gram_wgs + LFVIO_WINDOW_SIZE + 1, 1), dim3(LIN_THREADS), 0, ss, sh, back, mode,
                             lw_cap, gram_wgs, slot_args(L, back));  // (the shadow's variant: its input offsets lead back into slot 0)
        });
        hipLaunchKernelGGL(k_sum, dim3(HPP_BLOCKS + SCHUR_LEN / 256 + 1, 1), dim3(256), 0, ss, sh, back, mode, 0, sa);
        hipLaunchKernelGGL(k_marg_solve<true>, dim3(1, 1), dim3(MARG_THREADS), MARG_LDS, ss, sh, back,
                           p.marg_flag | (c->force_eig ? 256 : 0) | 512 | (p.publish ? 1024 : 0));
      }
      return LFVIO_OK;
    });
    if (rc) return rc;
  }
  return LFVIO_OK;
}

// The adaptive loop: the first graph, then — while a slot is open, the passes last and the wall clock allows — chunks, the host
// reading the PendingBlock in between.  *tail_done: the gated tail ran inside the first graph (or is running behind an early return)
int adaptive_loop(lfvio_ctx *c, const Route &r, const CallPlan &p, int passes, bool *tail_done) {
  const auto t_start = std::chrono::steady_clock::now();
  LoopGraphs G;
  if (int rc = loop_graphs(c, r, p, passes, &G)) return rc;
  const int count = r.count;
  const Grid &g = r.g;
  const bool fuse = p.fused, capped = p.max_seconds > 0.0;
  // Workers: one small window on the merged launch sequence (its loop ends in k_decide_gauge), with a shadow slot and a mailbox.
  // (not behind a device-chained upload: there the marginalization already runs beside the host's packing of the next window, and the next
  // window's upload would have to wait for a worker instead of following the stream)
  const bool ahead = fuse && count == 1 && c->info[0].spec_on && c->shadow && c->marg_ahead && !c->shard_active && !c->call.pipelined() &&
                     g.lm <= DOGLEG_INLINE_BLOCKS && g.ch_raw <= PRE_CHUNK_LIMIT && g.sc <= 4 * PRE_GROUP && r.sweep == Route::ROLES;
  if (ahead)
    if (int rc = worker_graphs(c, r, p)) return rc;
  // (ticket 0: a call without workers — rounds left over from an earlier call must not take its states: spec_publish)
  const int ticket = c->call.loop_started(ahead);
  if (c->h_mail && count == 1) *mail_word(c, MAIL_TICKET) = ticket;
  c->stat_chunks = 0;
  for (int done_passes = 0; done_passes < passes;) {
    c->stat_chunks++;
    const auto t_launch = std::chrono::steady_clock::now();
    const bool first = done_passes == 0;
    if (first) {
      bool early = false;
      const int rc = launch_watched(c, G.first, p.early && fuse && p.publish, &early, [&]() -> int {
        if (ahead) {  // (behind the loop's graph: on a shared hardware queue the workers would otherwise wait in front of it)
          for (int wk = 0; wk < lfvio_ctx::WORKERS; wk++) HIPCHK(c, hipGraphLaunch(c->side[wk][p.marg_flag][p.publish ? 1 : 0], c->sstream[wk]));
          c->call.workers_started(), c->stat_ahead_calls++;
        }
        if (c->call.pipelined()) c->up_us[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_launch).count() * 1e6;  // (debug: lfvio_debug_query "upload_times")
        return LFVIO_OK;
      });
      if (rc) return rc;
      if (early) {  // the window was done inside the first graph: its tail follows in the same graph.  The loop is closed: its counts size
                    // the next call's first graph (a caller that pipelines never joins this graph)
        record_mailbox_call(c, c->call.early_from_first());
        *tail_done = true;
        return LFVIO_OK;
      }
    } else
      HIPCHK(c, hipGraphLaunch(G.chunk, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    PendingBlock &hp = *c->h_pending;
    if (!first) {  // time per pass, for sizing a capped call's first graph (continuation chunks carry nothing but passes)
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_launch).count() / SOLVE_CHUNK;
      c->pass_seconds = 0.75 * c->pass_seconds + 0.25 * dt;
    }
    done_passes += first ? G.first_passes : SOLVE_CHUNK;
    if (first && fuse && count == 1) hp.open = hp.tail_state >= TAIL_DONE ? 0 : 1, hp.passes = hp.passes_used, c->last_iters = hp.iters_done;  // (TAIL_WORKER: the prior is a worker's)
    if (first && (c->call.first_graph_ended(fuse && count == 1, hp.open == 0) & CallState::CHECK_CHAIN_ERR) && hp.chain_err) {
      c->err = CHAIN_ERR_TEXT;
      return LFVIO_ERR_DEVICE;
    }
    if (hp.open == 0) {
      if (fuse && first) *tail_done = true;
      break;
    }
    if (capped && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= p.max_seconds) {
      // "Maximum solver time reached": the open slots end where they are, termination stays NO_CONVERGENCE
      hipLaunchKernelGGL(k_force_done, dim3((count + 63) / 64), dim3(64), 0, c->stream, c->d_base, c->L.total, count);
      HIPCHK(c, hipStreamSynchronize(c->stream));
      break;
    }
  }
  if (count == 1 && !*tail_done) {
    // the window was still open behind the first graph: the iters_done that graph copied is the upload's zero, and the tail graph that
    // sets it copies nothing back.  The count is final in the header (stream 0 is idle here); without it the next call would choose
    // its candidates from "no iterations" (loop_graphs) and "last_call" would report none (tests/test_spec_candidates.py).
    int it = 0;
    HIPCHK(c, hipMemcpy(&it, c->d_base + offsetof(Slot, tr) + offsetof(TRState, iteration), sizeof it, hipMemcpyDeviceToHost));
    c->last_iters = it;
  }
  record_call(c, c->h_pending->passes, c->last_iters, c->call.loop_ended());  // passes the slowest window has used
  HIPCHK(c, hipGetLastError());
  // (a call that ended inside its first graph: the prior may be on its way from a worker; one that continues with a tail graph
  // is waited for by the join in front of whatever comes next)
  if (*tail_done)
    if (int rc = wait_side(c)) return rc;
  return LFVIO_OK;
}

// Enqueue the trust-region loop for slots [0, p.count): max_iter Ceres iterations plus spare
// passes for mu-retries (a failed Cholesky consumes a pass but not an iteration).
//   adaptive = false: the whole loop as one static graph, nothing but enqueues (lfvio_batch_optimize_async).
//   adaptive = true (synchronous entry points): the passes go out in chunks of SOLVE_CHUNK and the host reads the number
//     of unfinished slots in between.  A pass costs its ~30 us of launches and first loads whether or not the loop is
//     already done, and with the speculative candidates of small windows nine iterations are four passes, not twelve.
// fused (adaptive only): gauge fix + marginalization ride in the graph of the first chunk, gated per slot on
// `done` — the common case (every window done within the first chunk) is ONE graph launch and one synchronization; *tail_done
// tells the caller whether anything is left for the (gated) tail graph.
// max_seconds > 0 (adaptive only): Ceres' max_solver_time_in_seconds (estimator.cpp:815-822) — TrustRegionMinimizer tests the
// wall clock at the top of every iteration and stops with NO_CONVERGENCE; here the host tests it between graph launches
// (the only points where it sees the loop) and ends the open slots the same way (k_force_done).  The first graph is sized
// from the previous call as without a cap, shortened only when the cap is tighter than that many passes would take.
// early (adaptive, fused, one window with a mailbox): return as soon as the solution is in the mailbox — the rest of the graph
// (the marginalization) is still running then and c->call says so.
int enqueue_solve(lfvio_ctx *c, const CallPlan &p, bool *tail_done) {
  *tail_done = false;
  if (int rc = join_inflight(c, p.early ? CallState::OVERTAKE_PIPELINED : CallState::WAIT)) return rc;
  const Route r = route_for(c, p.count, MODE_SOLVE);
  const int passes = std::max(p.max_iter, 0) + 4;
  if (p.adaptive && c->use_graph) return adaptive_loop(c, r, p, passes, tail_done);
  launch_setup(c, r, MODE_SOLVE);
  // (the pass behind k_setup sweeps at the uploaded state: slots_offs)
  auto loop = [&]() {
    Pass ps;
    for (int it = 0; it < passes; it++) {
      ps.first = it == 0, ps.last = it == passes - 1, ps.offs = (r.offs & 2) || (it == 0 && (r.offs & 1));
      launch_iteration(c, r, MODE_SOLVE, ps);
    }
    return LFVIO_OK;
  };
  if (c->use_graph) {
    const GraphKey key = graph_key(r, 0, passes, false);  // (k_setup goes out in front of this graph)
    if (!c->graph || !(c->graph_key == key)) {
      if (c->graph) (void)hipGraphExecDestroy(c->graph), c->graph = nullptr;
      if (int rc = capture_graph(c, c->stream, &c->graph, loop)) return rc;
      c->graph_key = key;
    }
    HIPCHK(c, hipGraphLaunch(c->graph, c->stream));
  } else {
    loop();
  }
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

int enqueue_marg(lfvio_ctx *c, const CallPlan &p, MargKind kind) {
  const bool gated = kind == MARG_GATED, standalone = kind == MARG_STANDALONE;
  if (int rc = join_inflight(c, gated ? CallState::OVERTAKE_PIPELINED : CallState::WAIT)) return rc;  // (gated: part of a graph of lfvio_batch_optimize*, which has joined — or may go out behind a pipelined upload)
  const int flag = p.marg_flag, mode = (MODE_MARG + flag) | (gated ? MODE_GATED : 0);
  const Route r = route_for(c, p.count, mode);
  if (standalone) launch_setup(c, r, mode);
  // (standalone: the sweep is at the uploaded state; gated: at the re-anchored solution, on the sphere but for a fixed extrinsic)
  Pass ps;
  ps.offs = standalone ? r.offs != 0 : (r.offs & 2) != 0;
  launch_iteration(c, r, mode, ps);
  hipLaunchKernelGGL(k_marg_solve<false>, dim3(1, p.count), dim3(MARG_THREADS), MARG_LDS, c->stream, c->d_base, c->L.total,
                     flag | (c->force_eig ? 256 : 0) | (gated ? 512 : 0) | (gated && p.publish ? 1024 : 0));
  HIPCHK(c, hipGetLastError());
  return LFVIO_OK;
}

// Results come back through one pinned block [x[2] | tr | lam[0] | lam[1] | prior]: every copy a call needs is enqueued and
// the stream is synchronized ONCE (a round trip costs ~12 us; the drop-in call used to make four).  Which of the two
// inverse-depth buffers is current is only known from `tr`, so small windows fetch both; windows beyond ONE_TRIP_LM
// landmarks take a second trip for the one that matters instead of moving megabytes for nothing.
constexpr int ONE_TRIP_LM = 8192;
struct Fetched {
  const FrameState *xs;
  const TRState *tr;
  const double *lam[2];
  LfvioPrior *prior;
};

int fetch(lfvio_ctx *c, int slot, bool want_sol, bool want_prior, Fetched *f) {
  if (int rc = join_inflight(c)) return rc;
  const Layout &L = c->L;
  char *d = c->d_base + (size_t)slot * L.total;
  const SlotHostInfo &info = c->info[slot];
  if (!info.resident) {
    c->err = "slot not uploaded";
    return LFVIO_ERR_ARG;
  }
  char *hd = c->h_down;
  const size_t hdr = sizeof(FrameState) * 2 + sizeof(TRState), lam_bytes = (size_t)info.N * 8;
  char *h_lam0 = hd + hdr, *h_lam1 = h_lam0 + align_up(lam_bytes + 8, 64), *h_prior = h_lam1 + align_up(lam_bytes + 8, 64);
  f->xs = (const FrameState *)hd, f->tr = (const TRState *)(hd + sizeof(FrameState) * 2);
  f->lam[0] = (const double *)h_lam0, f->lam[1] = (const double *)h_lam1, f->prior = (LfvioPrior *)h_prior;
  const bool both = info.N > 0 && info.N <= ONE_TRIP_LM;
  if (want_sol) {
    HIPCHK(c, hipMemcpyAsync(hd, d + offsetof(Slot, x), hdr, hipMemcpyDeviceToHost, c->stream));
    if (both) {
      HIPCHK(c, hipMemcpyAsync(h_lam0, d + L.lam[0], lam_bytes, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(h_lam1, d + L.lam[1], lam_bytes, hipMemcpyDeviceToHost, c->stream));
    }
  }
  if (want_prior) {
    // the dimension of the prior a marginalization of this window can produce is known since the upload (plan_marg)
    const size_t head = offsetof(LfvioPrior, linearized_jacobians), n = (size_t)info.marg_n;
    HIPCHK(c, hipMemcpyAsync(h_prior, d + offsetof(Slot, prior_out), head + sizeof(double) * n * n, hipMemcpyDeviceToHost, c->stream));
    if (n)
      HIPCHK(c, hipMemcpyAsync(h_prior + offsetof(LfvioPrior, linearized_residuals), d + offsetof(Slot, prior_out) + offsetof(LfvioPrior, linearized_residuals),
                               sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (want_sol && !both && info.N > 0 && !f->tr->error) {
    HIPCHK(c, hipMemcpyAsync(f->tr->cur ? h_lam1 : h_lam0, d + L.lam[f->tr->cur], lam_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return LFVIO_OK;
}

// nothing is written to the caller's outputs before the result is known to be usable (the header promises untouched
// outputs on error): check_* first, then unpack_*.  The solution of a loop: its header tr, the state x[tr->cur] (nx doubles:
// a FrameState, or the relo route's ReloX), lam[tr->cur] (N inverse depths, device order; perm[dl]: the caller's index,
// nullptr: the caller's order)
int check_solution(lfvio_ctx *c, const TRState *tr, const double *x, int nx, const double *lam, int N) {
  if (tr->error) {
    c->err = "non-finite cost";
    return tr->error;
  }
  bool finite = std::isfinite(tr->x_cost);
  for (int k = 0; finite && k < nx; k++) finite = std::isfinite(x[k]);
  for (int dl = 0; finite && dl < N; dl++) finite = std::isfinite(lam[dl]);
  if (!finite) {
    c->err = "non-finite state";
    return LFVIO_ERR_NONFINITE;
  }
  return LFVIO_OK;
}

void unpack_solution(const TRState *tr, const FrameState &x, const double *lam, int N, const int *perm, LfvioSolution *out) {
  std::memcpy(out->para_pose, x.pose, sizeof x.pose);
  std::memcpy(out->para_speed_bias, x.sb, sizeof x.sb);
  std::memcpy(out->para_ex_pose, x.ex, sizeof x.ex);
  out->para_td = x.td;
  if (out->inv_depth)
    for (int dl = 0; dl < N; dl++) out->inv_depth[perm ? perm[dl] : dl] = lam[dl];
  out->num_iterations = tr->trace_len;
  out->num_successful_steps = tr->num_succ;
  out->num_unsuccessful_steps = tr->num_unsucc;
  out->termination = tr->termination;
  out->initial_cost = tr->initial_cost;
  out->final_cost = tr->x_cost;
  std::memset(out->trace, 0, sizeof out->trace);
  for (int k = 0; k < tr->trace_len && k < LFVIO_MAX_TRACE; k++) out->trace[k] = tr->trace[k];
}

// returns LFVIO_OK with *pass = true when nothing was marginalized and the input prior stays
int check_prior(lfvio_ctx *c, int slot, const Fetched &f, bool *pass) {
  const SlotHostInfo &info = c->info[slot];
  const LfvioPrior *hp = f.prior;
  *pass = hp->valid == -1;
  if (*pass) return LFVIO_OK;
  const int n = hp->n;
  // (n = 0: a marginalization in which nothing takes part — no prior, IMU interval 0 skipped, no landmark anchored at frame 0 — leaves a
  // valid prior with m = n = 0 and no blocks, as the oracle's statement of MarginalizationInfo::marginalize does)
  if (hp->valid != 1 || n < 0 || n > LFVIO_MAX_PRIOR_DIM || n > info.marg_n) {
    c->err = "marginalization produced no prior";
    return LFVIO_ERR_DEVICE;
  }
  bool finite = true;
  for (int k = 0; finite && k < n * n; k++) finite = std::isfinite(hp->linearized_jacobians[k]);
  for (int k = 0; finite && k < n; k++) finite = std::isfinite(hp->linearized_residuals[k]);
  if (!finite) {
    c->err = "non-finite prior";
    return LFVIO_ERR_NONFINITE;
  }
  return LFVIO_OK;
}

void unpack_prior(lfvio_ctx *c, int slot, const Fetched &f, bool pass, LfvioPrior *out) {
  const SlotHostInfo &info = c->info[slot];
  if (pass) {
    if (info.has_in_prior) copy_prior(out, &info.in_prior);
    else out->valid = 0;
    return;  // (a prior whose values stayed on the device: fetch_device_prior below, by the callers that can synchronize)
  }
  const LfvioPrior *hp = f.prior;
  const int n = hp->n;
  std::memcpy(out, hp, offsetof(LfvioPrior, linearized_jacobians));
  std::memcpy(out->linearized_jacobians, hp->linearized_jacobians, sizeof(double) * n * n);
  std::memcpy(out->linearized_residuals, hp->linearized_residuals, sizeof(double) * n);
}

// The input prior of a window that took it over on the device (lfvio_batch_upload_chained_device) and whose own marginalization
// passes it through: its values have never been on the host — they are read out of the slot now (a synchronization and three
// small copies, in a case the reference meets once per MARGIN_SECOND_NEW without a prior on the newest pose).
int fetch_device_prior(lfvio_ctx *c, int slot, LfvioPrior *out) {
  SlotHostInfo &info = c->info[slot];
  if (!info.in_prior_device) return LFVIO_OK;
  const char *d = c->d_base + (size_t)slot * c->L.total;
  LfvioPrior *p = &info.in_prior;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(p->linearized_jacobians, d + c->L.prior_J, sizeof(double) * p->n * p->n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(p->linearized_residuals, d + c->L.prior_r, sizeof(double) * p->n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(p->block_x0, d + offsetof(Slot, prior_x0), sizeof(double) * 9 * p->num_blocks, hipMemcpyDeviceToHost));
  info.in_prior_device = false;
  if (out) copy_prior(out, p);
  return LFVIO_OK;
}

int download(lfvio_ctx *c, int slot, LfvioSolution *sol, LfvioPrior *prior) {
  Fetched f;
  int rc = fetch(c, slot, sol != nullptr, prior != nullptr, &f);
  if (rc) return rc;
  bool pass = false;
  const SlotHostInfo &info = c->info[slot];
  const int cur = sol ? f.tr->cur : 0;
  if (sol && (rc = check_solution(c, f.tr, (const double *)&f.xs[cur], sizeof(FrameState) / 8, f.lam[cur], info.N))) return rc;
  if (prior && (rc = check_prior(c, slot, f, &pass))) return rc;
  if (sol) unpack_solution(f.tr, f.xs[cur], f.lam[cur], info.N, info.perm.data(), sol);
  if (prior && pass && (rc = fetch_device_prior(c, slot, nullptr))) return rc;
  if (prior) unpack_prior(c, slot, f, pass, prior);
  return LFVIO_OK;
}
int download_solution(lfvio_ctx *c, int slot, LfvioSolution *out) { return download(c, slot, out, nullptr); }
int download_prior(lfvio_ctx *c, int slot, LfvioPrior *out) { return download(c, slot, nullptr, out); }

}  // namespace

extern "C" {

const char *lfvio_version(void) { return "lfvio-hip 0.1 (gfx950, FP64)"; }

lfvio_ctx *lfvio_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  lfvio_ctx *c = new lfvio_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return nullptr;
  }
  {
    // The stream of the feature steps must not share a hardware queue with `stream`, or its kernels wait behind the tail they
    // are meant to run beside: the runtime deals its (four, by default) hardware queues to streams round-robin PER PRIORITY
    // LEVEL, so with a second context in the process the two streams of one context can land on the same queue (measured:
    // lfvio_shift_depth 45 us -> 216 us behind a marginalization).  A stream of another priority comes from another pool.
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&c->fstream, hipStreamNonBlocking, greatest) != hipSuccess) c->fstream = nullptr;  // (falls back to `stream`)
    // ... and the workers of the marginalization run ahead (kernels_spec.h) from the third pool; without three levels there are none
    for (int wk = 0; wk < lfvio_ctx::WORKERS; wk++)
      if (least == greatest || hipStreamCreateWithPriority(&c->sstream[wk], hipStreamNonBlocking, least) != hipSuccess) c->sstream[wk] = nullptr;
  }
  // the mailbox: fine-grained host memory mapped into the device's address space.  Without it begin() simply waits for the end.
  if (c->h_mail.reserve(MAIL_BYTES)) {
    std::memset(c->h_mail, 0, MAIL_BYTES);
    if (hipHostGetDevicePointer((void **)&c->d_mail, c->h_mail, 0) != hipSuccess) c->d_mail = nullptr;
  } else {
    (void)hipGetLastError();
  }
  // kernels that need more than the default 64 KiB of LDS
  (void)hipFuncSetAttribute((const void *)k_solve_dense<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SOLVE_LDS);
  (void)hipFuncSetAttribute((const void *)k_solve_dense<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SOLVE_LDS);
  (void)hipFuncSetAttribute((const void *)k_linw<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LW_LDS_BYTES);
  (void)hipFuncSetAttribute((const void *)k_linw<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LW_LDS_BYTES);
  (void)hipFuncSetAttribute((const void *)k_linb<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LW_LDS_BYTES);
  (void)hipFuncSetAttribute((const void *)k_linb<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LW_LDS_BYTES);
  {  // static table of k_linw's phase 3: where each packed camera entry of H_pp (then each camera-side gradient entry) sits in the LDS accumulators
    std::vector<int> tab(SUM_VIS);
    for (int e = 0; e < SUM_VIS; e++) {
      int r, cc;
      if (e < SUM_VIS_PACKED) {
        r = 0;
        while ((r + 1) * (r + 2) / 2 <= e) r++;
        cc = e - r * (r + 1) / 2;
      } else {
        r = cc = e - SUM_VIS_PACKED;
      }
      const int fr = r < 66 ? r / 6 : 11, fc = cc < 66 ? cc / 6 : 11, lr = r < 66 ? r - 6 * fr : r - 66, lc = cc < 66 ? cc - 6 * fc : cc - 66;
      int at;
      if (e >= SUM_VIS_PACKED) at = LW_G + cc;
      else if (fr == fc && fr < 11) at = LW_D + 21 * fr + lw_tri(6, lc, lr);
      else if (fr < 11) at = (LW_OFF0 + 36 * lw_pidx(fc, fr) + lc * 6 + lr) | LWT_ABS | (fc << 20) | (fr << 24);  // (frames of the block: k_linb)
      else if (fc < 11) at = LW_FX + 42 * fc + lc * 7 + lr;
      else at = LW_XX + lw_tri(7, lc, lr);
      auto is_ex = [](int q) { return q >= 66 && q < 72; };
      if (is_ex(r) || is_ex(cc)) at |= LWT_EX;
      if (r == 72 || cc == 72) at |= LWT_TD;
      tab[e] = at;
    }
    if (!c->d_lwt.reserve(sizeof(int) * tab.size()) ||
        hipMemcpy(c->d_lwt, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
      lfvio_destroy(c);
      return nullptr;
    }
  }
  {  // static scatter table of the assembling solve: packed visual entry -> tile address; IMU block entries, even factors then odd
    std::vector<int> tab(ASM_LEN);
    for (int r = 0, e = 0; r < KC; r++)
      for (int cc = 0; cc <= r; cc++, e++) tab[e] = asm_lidx(r, cc);
    auto glob = [](int p, int f) { return p < 6 ? 6 * f + p : p < 15 ? KC + 9 * f + (p - 6) : p < 21 ? 6 * (f + 1) + (p - 15) : KC + 9 * (f + 1) + (p - 21); };
    for (int par = 0; par < 2; par++) {
      std::vector<std::pair<int, int>> ent;  // (tile address, source index)
      for (int f = par; f < LFVIO_WINDOW_SIZE; f += 2)
        for (int p = 0; p < 30; p++)
          for (int q = 0; q < 30; q++)
            if (glob(p, f) >= glob(q, f)) ent.push_back({asm_lidx(glob(p, f), glob(q, f)), f * IMU_OUT + p * 30 + q});
      std::sort(ent.begin(), ent.end());
      for (size_t k = 0; k < ent.size(); k++) tab[ASM_VIS + par * ASM_IMU_HALF + k] = ent[k].second | (ent[k].first << 16);
    }
    if (!c->d_asm.reserve(sizeof(int) * tab.size()) ||
        hipMemcpy(c->d_asm, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
      lfvio_destroy(c);
      return nullptr;
    }
  }
  (void)hipFuncSetAttribute((const void *)k_relo_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RELO_SOLVE_LDS);
  (void)hipFuncSetAttribute((const void *)k_marg_solve<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MARG_LDS);
  (void)hipFuncSetAttribute((const void *)k_marg_solve<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MARG_LDS);
  return c;
}

void lfvio_destroy(lfvio_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  destroy_graph(c);
  delete c;  // the buffers, then the events and streams (CtxQueues)
}

const char *lfvio_last_error(const lfvio_ctx *c) { return c ? c->err.c_str() : "null context"; }
void *lfvio_stream(lfvio_ctx *c) { return c ? (void *)c->stream : nullptr; }

int lfvio_solve(lfvio_ctx *c, const LfvioWindow *in, LfvioSolution *out) {
  if (!c || !in || !out) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  int rc = reserve(c, 1, in->num_landmarks, in->num_observations);
  if (rc) return rc;
  if ((rc = upload_window(c, 0, in))) return rc;
  CallPlan p;
  p.max_iter = in->max_num_iterations, p.max_seconds = in->max_solver_time_in_seconds;
  bool tail_done = false;
  if ((rc = enqueue_solve(c, p, &tail_done))) return rc;
  return download_solution(c, 0, out);
}

int lfvio_marginalize(lfvio_ctx *c, const LfvioWindow *in, int flag, LfvioPrior *out) {
  if (!c || !in || !out || (flag != LFVIO_MARGIN_OLD && flag != LFVIO_MARGIN_SECOND_NEW)) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  int rc = reserve(c, 1, in->num_landmarks, in->num_observations);
  if (rc) return rc;
  if ((rc = upload_window(c, 0, in))) return rc;
  CallPlan p;
  p.marg_flag = flag;
  if ((rc = enqueue_marg(c, p, MARG_STANDALONE))) return rc;
  return download_prior(c, 0, out);
}

int lfvio_batch_reserve(lfvio_ctx *c, int batch, int max_landmarks, int max_observations) {
  if (!c || batch <= 0) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  return reserve(c, batch, max_landmarks, max_observations);
}

int lfvio_batch_upload(lfvio_ctx *c, int slot, const LfvioWindow *in) {
  if (!c || !in || slot < 0 || slot >= c->batch) return LFVIO_ERR_ARG;
  if (in->num_landmarks > c->L.maxN || in->num_observations > c->L.maxM) {
    c->err = "window larger than the reserved capacity";
    return LFVIO_ERR_ARG;
  }
  (void)hipSetDevice(c->device);
  return upload_window(c, slot, in);
}

int lfvio_batch_upload_chained_device(lfvio_ctx *c, int slot, const LfvioWindow *in) {
  if (!c || !in || slot < 0 || slot >= c->batch) return LFVIO_ERR_ARG;
  if (in->num_landmarks > c->L.maxN || in->num_observations > c->L.maxM) {
    c->err = "window larger than the reserved capacity";
    return LFVIO_ERR_ARG;
  }
  (void)hipSetDevice(c->device);
  UploadMode mode;
  mode.device_chain = true;
  return upload_window(c, slot, in, mode);
}

int lfvio_batch_upload_chained(lfvio_ctx *c, int slot, const LfvioWindow *in, LfvioPrior *prior_io) {
  if (!c || !in || !prior_io || slot < 0 || slot >= c->batch) return LFVIO_ERR_ARG;
  if (in->num_landmarks > c->L.maxN || in->num_observations > c->L.maxM) {
    c->err = "window larger than the reserved capacity";
    return LFVIO_ERR_ARG;
  }
  (void)hipSetDevice(c->device);
  UploadMode mode;
  mode.chain = prior_io;
  return upload_window(c, slot, in, mode);
}

enum CallForm { CALL_STATIC, CALL_ADAPTIVE, CALL_EARLY };  // lfvio_batch_optimize_async | lfvio_batch_optimize | lfvio_batch_optimize_begin
static int batch_optimize_impl(lfvio_ctx *c, int count, int marg_flag, CallForm form) {
  if (!c || count <= 0 || count > c->batch) return LFVIO_ERR_ARG;
  if (marg_flag != LFVIO_MARGIN_OLD && marg_flag != LFVIO_MARGIN_SECOND_NEW) {  // (the flag indexes the slot's two marginalization plans)
    c->err = "marg_flag is neither LFVIO_MARGIN_OLD nor LFVIO_MARGIN_SECOND_NEW";
    return LFVIO_ERR_ARG;
  }
  (void)hipSetDevice(c->device);
  CallPlan p;
  p.count = count, p.marg_flag = marg_flag, p.adaptive = form != CALL_STATIC, p.early = form == CALL_EARLY;
  if (int rc = join_inflight(c, p.early && count == 1 ? CallState::OVERTAKE_PIPELINED : CallState::WAIT)) return rc;
  c->call.optimize_started(marg_flag);
  p.publish = p.early && count == 1 && c->h_mail && c->info[0].resident && c->info[0].N <= MAIL_MAX_LM;
  // every slot carries its own max_iter on the device; the pass count follows the largest, the wall-clock cap
  // (synchronous driver only) the smallest positive one
  for (int s = 0; s < count; s++) {
    if (!c->info[s].resident) {
      c->err = "slot not uploaded";
      return LFVIO_ERR_ARG;
    }
    p.max_iter = std::max(p.max_iter, c->info[s].max_iter);
    const double t = c->info[s].max_seconds;
    if (t > 0.0 && (p.max_seconds <= 0.0 || t < p.max_seconds)) p.max_seconds = t;
  }
  if (c->info[0].in_prior_device && (count != 1 || !p.adaptive || !c->use_graph)) {
    // (k_prior_chain's verdict on the prior travels with the graph of ONE window's synchronous call: include/lfvio.h)
    c->err = "a window uploaded with lfvio_batch_upload_chained_device is optimized by lfvio_batch_optimize_begin or lfvio_batch_optimize(ctx, 1, flag)";
    return LFVIO_ERR_ARG;
  }
  p.fused = p.adaptive && c->use_graph;
  bool tail_done = false;
  int rc = enqueue_solve(c, p, &tail_done);
  if (rc) return rc;
  if (p.fused) {
    if (tail_done) return LFVIO_OK;  // the usual case: everything ran in the graph of the first chunk
    // some window needed more passes: gauge fix + marginalization for the slots that have not had theirs (gated)
    hipGraphExec_t &tail_graph = c->tail[p.publish ? 1 : 0][marg_flag];
    if (!tail_graph) {
      rc = capture_graph(c, c->stream, &tail_graph, [&]() {
        hipLaunchKernelGGL(k_force_done, dim3((count + 63) / 64), dim3(64), 0, c->stream, c->d_base, c->L.total, count);
        hipLaunchKernelGGL(k_gauge, dim3(1 + (grid_for(c, count).lm + 1) / 2, count), dim3(128), 0, c->stream, c->d_base, c->L.total, 1);
        if (p.publish) hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, c->stream, c->d_base, c->L.total);
        return enqueue_marg(c, p, MARG_GATED);
      });
      if (rc) return rc;
    }
    bool early = false;
    if ((rc = launch_watched(c, tail_graph, p.publish, &early, [] { return LFVIO_OK; }))) return rc;
    if (early) record_mailbox_call(c, c->call.early_from_tail());
    return LFVIO_OK;
  }
  hipLaunchKernelGGL(k_gauge, dim3(1 + (grid_for(c, count).lm + 1) / 2, count), dim3(128), 0, c->stream, c->d_base, c->L.total, 0);
  return enqueue_marg(c, p, MARG_AFTER_LOOP);
}

int lfvio_batch_optimize_async(lfvio_ctx *c, int count, int marg_flag) { return batch_optimize_impl(c, count, marg_flag, CALL_STATIC); }

int lfvio_batch_sync(lfvio_ctx *c) {
  if (!c) return LFVIO_ERR_ARG;
  if (int rc = join_inflight(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return wait_side(c);
}

int lfvio_batch_optimize(lfvio_ctx *c, int count, int marg_flag) {
  int rc = batch_optimize_impl(c, count, marg_flag, CALL_ADAPTIVE);
  if (rc) return rc;
  return lfvio_batch_sync(c);
}

int lfvio_batch_download(lfvio_ctx *c, int slot, LfvioSolution *sol, LfvioPrior *prior) {
  if (!c || slot < 0 || slot >= c->batch) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  return download(c, slot, sol, prior);
}

// The split form of lfvio_batch_optimize(ctx, 1, marg_flag) + lfvio_batch_download(ctx, 0, sol, prior) for ONE resident window:
// begin() returns with the solution as soon as solve + gauge fix are out — the gated gauge fix pushes the state into host
// memory (Slot::mail) and the host polls that word, no copy and no stream synchronization — while the marginalization of the
// same graph is still running; finish() waits for it and fetches the prior.  (estimator.cpp: the pose is published after
// optimization(), the prior is first read by the next optimization(): the ~0.19 ms of the marginalization overlap with
// whatever the caller does in between.)  Windows without a mailbox (more than MAIL_MAX_LM landmarks, no mapped host memory)
// and windows that were not done within the first graph take the synchronous route inside begin().
int lfvio_batch_optimize_begin(lfvio_ctx *c, int marg_flag, LfvioSolution *sol) {
  if (!c || !sol || c->batch < 1) return LFVIO_ERR_ARG;
  int rc = batch_optimize_impl(c, 1, marg_flag, CALL_EARLY);
  if (rc) return rc;
  if (!c->call.early()) return download(c, 0, sol, nullptr);  // (synchronizes)
  Fetched f;
  char *m = c->h_mail;
  if (*mail_word(c, MAIL_CHAIN_ERR)) {  // (CHECK_CHAIN_ERR of the early return: said here, with the state, and by no join after it)
    c->err = CHAIN_ERR_TEXT;
    return LFVIO_ERR_DEVICE;
  }
  f.xs = (const FrameState *)(m + MAIL_X), f.tr = (const TRState *)(m + MAIL_TR);
  f.lam[0] = (const double *)(m + MAIL_LAM), f.lam[1] = (const double *)(m + MAIL_LAM + MAIL_LAM_STRIDE), f.prior = nullptr;
  const int cur = f.tr->cur, N = c->info[0].N;
  if ((rc = check_solution(c, f.tr, (const double *)&f.xs[cur], sizeof(FrameState) / 8, f.lam[cur], N))) return rc;
  unpack_solution(f.tr, f.xs[cur], f.lam[cur], N, c->info[0].perm.data(), sol);
  return LFVIO_OK;
}

int lfvio_batch_optimize_finish(lfvio_ctx *c, LfvioPrior *prior) {
  if (!c) return LFVIO_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (c->call.held_handed_out()) {
    if (prior) copy_prior(prior, c->held.get());
    return LFVIO_OK;
  }
  if (c->call.early() && prior) {
    // the marginalization ends by pushing its prior into the mailbox (publish_prior): wait for that word, not for the stream
    int *flag = (int *)c->h_mail.get() + MAIL_PRIOR_FLAG;
    const int want = c->info[0].mail_seq;
    bool there = false;
    for (;;) {
      if ((there = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == want)) break;
      if (hipStreamQuery(c->stream) != hipErrorNotReady && !(c->call.workers_outstanding() && (hipStreamQuery(c->sstream[0]) == hipErrorNotReady || hipStreamQuery(c->sstream[1]) == hipErrorNotReady))) {
        there = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == want;  // (a worker of kernels_spec.h may still be delivering when stream 0 is idle)
        break;
      }
    }
    if (there) {
      c->call.prior_from_mailbox();  // (what is left of the graph is a copy of two words: the next join waits for it)
      record_call(c, *mail_word(c, MAIL_PRIOR_PASSES), *mail_word(c, MAIL_PRIOR_ITERS), CallState::NOTHING);
      Fetched f{};
      f.prior = (LfvioPrior *)(c->h_mail + MAIL_PRIOR);
      bool pass = false;
      if (int rc = check_prior(c, 0, f, &pass)) return rc;
      if (pass)
        if (int rc = fetch_device_prior(c, 0, nullptr)) return rc;
      unpack_prior(c, 0, f, pass, prior);
      return LFVIO_OK;
    }
  }
  int rc = join_inflight(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return prior ? download(c, 0, nullptr, prior) : LFVIO_OK;
}

int lfvio_batch_optimize_pending(const lfvio_ctx *c) { return c && c->call.pending() ? 1 : 0; }

// ---- debug / parity hooks: declared in lfvio_debug.h, implemented in debug.inc
#include "debug.inc"
// ---- relocalization: lfvio_solve_relo, declared in lfvio.h, implemented in relo.inc
#include "relo.inc"
// ---- the calls on the feature stream: feat.inc holds their staging and the three feature steps
#include "feat.inc"

#include "twoview.inc"
#include "relpose.inc"

#include "vialign.inc"

#include "pnp.inc"

#include "sfmba.inc"

#include "sfmchain.inc"

#include "clahe.inc"

#include "imgfmt.inc"

#include "remap.inc"

#include "fuse.inc"

#include "tracksource.inc"

#include "klt.inc"

#include "gft.inc"

#include "track.inc"

#include "trackframe.inc"

#include "trackbatch.inc"
// ---- landmark-sharded API: declared in lfvio.h, implemented in shard.inc
#include "shard.inc"
// ---- multi-GPU groups (RCCL): declared in lfvio.h, implemented in group.inc
#include "group.inc"

}  // extern "C"
