// window_pack.h — host packing of one LfvioWindow into the staging copy of a slot blob (dev_types.h, slot_args.h): where the device's
// data layout is PRODUCED.  Plain C++ (no HIP): lfvio_hip.hip packs every upload with it, tests/test_window_pack.py compiles this file
// alone and checks the order of landmarks and observations, the chunks, strips, gather lists and marginalization plans on the CPU.
//
// pack_window() writes everything that does not depend on the window's prior, pack_prior() the rest: an upload chained behind a call in
// flight (lfvio_batch_upload_chained) collects that call's prior between the two.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "slot_args.h"
#include "linb_plan.h"

inline int local_size(int kind) {
  return (kind == LFVIO_BLOCK_POSE || kind == LFVIO_BLOCK_EX_POSE) ? 6 : (kind == LFVIO_BLOCK_SPEEDBIAS ? 9 : 1);
}
inline int tangent_off(int kind, int frame) {
  return kind == LFVIO_BLOCK_POSE ? off_pose(frame)
         : kind == LFVIO_BLOCK_SPEEDBIAS ? off_sb(frame)
         : kind == LFVIO_BLOCK_EX_POSE ? off_ex()
                                       : off_td();
}

// Structure of MarginalizationInfo for this window (estimator.cpp:833-1005): which blocks
// take part, which are dropped, canonical column order (dropped first, then poses / speed-bias
// by frame, ex pose, td) and the addr_shift of the kept blocks.
// N0 / nChunks0: what THIS slot sweeps; any0 / kmax0: whether the WINDOW has landmarks anchored at frame 0 and their longest track —
// the same thing unless the slot holds a rank's share of a landmark-sharded window, whose block structure is the whole window's
inline void plan_marg(const LfvioWindow *w, const LfvioPrior *pr, int flag, int N0, bool any0, int kmax0, int nChunks0, bool imu0_ok, MargPlan *mp) {
  std::memset(mp, 0, sizeof *mp);
  for (int c = 0; c < KP; c++) mp->col[c] = -1;
  bool present[4][LFVIO_NUM_FRAMES] = {}, dropped[4][LFVIO_NUM_FRAMES] = {};
  auto touch = [&](int kind, int frame, bool drop) {
    present[kind][frame] = true;
    if (drop) dropped[kind][frame] = true;
  };
  if (flag == LFVIO_MARGIN_OLD) {
    if (pr)
      for (int i = 0; i < pr->num_blocks; i++) {
        const int k = pr->blocks[i].kind, f = pr->blocks[i].frame;
        touch(k, f, (k == LFVIO_BLOCK_POSE || k == LFVIO_BLOCK_SPEEDBIAS) && f == 0);
      }
    mp->use_imu0 = (w->imu[0].sum_dt < 10.0) && imu0_ok;
    if (w->imu[0].sum_dt < 10.0) {
      touch(LFVIO_BLOCK_POSE, 0, true), touch(LFVIO_BLOCK_SPEEDBIAS, 0, true);
      touch(LFVIO_BLOCK_POSE, 1, false), touch(LFVIO_BLOCK_SPEEDBIAS, 1, false);
    }
    if (any0) {
      touch(LFVIO_BLOCK_POSE, 0, true);
      for (int j = 1; j < kmax0; j++) touch(LFVIO_BLOCK_POSE, j, false);
      touch(LFVIO_BLOCK_EX_POSE, 0, false);
      if (w->estimate_td) touch(LFVIO_BLOCK_TD, 0, false);
    }
    mp->N0 = N0;
    mp->nChunks0 = nChunks0;
    mp->use_visual = N0 > 0;
    mp->valid = 1;
  } else {
    bool touches = false;
    if (pr)
      for (int i = 0; i < pr->num_blocks; i++)
        if (pr->blocks[i].kind == LFVIO_BLOCK_POSE && pr->blocks[i].frame == LFVIO_WINDOW_SIZE - 1) touches = true;
    if (!touches) return;  // valid = 0
    for (int i = 0; i < pr->num_blocks; i++) {
      const int k = pr->blocks[i].kind, f = pr->blocks[i].frame;
      touch(k, f, k == LFVIO_BLOCK_POSE && f == LFVIO_WINDOW_SIZE - 1);
    }
    mp->valid = 1;
  }
  int pos = 0;
  for (int k = 0; k < 4; k++)
    for (int f = 0; f < LFVIO_NUM_FRAMES; f++)
      if (present[k][f] && dropped[k][f]) {
        const int o = tangent_off(k, f);
        for (int e = 0; e < local_size(k); e++) mp->col[o + e] = pos++;
      }
  mp->m15 = pos;
  int nb = 0;
  for (int k = 0; k < 4; k++)
    for (int f = 0; f < LFVIO_NUM_FRAMES; f++)
      if (present[k][f] && !dropped[k][f]) {
        const int o = tangent_off(k, f);
        mp->kind[nb] = k, mp->frame[nb] = f, mp->idx[nb] = pos - mp->m15;
        int sf = f;
        if (k == LFVIO_BLOCK_POSE || k == LFVIO_BLOCK_SPEEDBIAS) {
          if (flag == LFVIO_MARGIN_OLD) sf = f - 1;
          else if (f == LFVIO_WINDOW_SIZE) sf = LFVIO_WINDOW_SIZE - 1;
        }
        mp->shifted_frame[nb] = sf;
        nb++;
        for (int e = 0; e < local_size(k); e++) mp->col[o + e] = pos++;
      }
  mp->nb = nb;
  mp->n = pos - mp->m15;
}

// What pack_window takes from the context that uploads (lfvio_ctx), beside the window and the layout
struct PackOptions {
  int slot = 0;
  int sharded = 0, pose_side = 1;  // Slot::sharded, Slot::pose_side
  long long mail = 0;              // device address of the context's mailbox (0: none); slot 0 of an unsharded window up to MAIL_MAX_LM gets it
  bool shadow = false;             // the context keeps shadow slots behind its last one ...
  bool marg_ahead = false;         // ... and may run the marginalization ahead in them (Slot::spec_on)
  int lm_half = 1;                 // 8 lanes per track in k_lin's landmark role where the window is small enough
  bool want_linw = false;          // plan the strips of k_linw (dropped where the window has more than LINW_MAX_STRIPS)
  bool want_linb = false;          // plan the groups of k_linb (dropped where they outnumber the Schur partials' space)
  int linb_max_groups = 0;
  double fn_tol = 1e-6, init_radius = 1e4;
  int seq = 1;                     // Slot::mail_seq
};

struct PackResult {
  int N = 0, M = 0;
  int N0 = 0, kmax0 = 0;  // landmarks anchored at frame 0 (a prefix of the device order), their longest track
  int nChunks = 0;
  bool linw = false, linb = false;  // the block carries a strip plan with its arrays | a group plan
  int linb_ng = 0;
  int used_items = 0;         // entries of sum_items the lists take ...
  bool lists_cached = false;  // ... which the device still holds from the slot's last upload: sum_off .. sum_items were not written
  bool offs_first = false, offs_all = false;  // SlotHostInfo: a quaternion of the start state is off the unit sphere
};

// The packing of one window, a method per section; every section reads what the ones before it left in the block.
struct WindowPacker {
  const LfvioWindow *w;
  const Layout &L;
  char *h;
  Slot *S;
  PackResult &r;
  int pair_count[NPAIR + 1] = {0};  // prefix sums: first pair-major observation of every frame pair

  template <class T>
  T *at(size_t off) const { return (T *)(h + off); }

  // ---- the slot header's scalars and the start state
  void header(const PackOptions &opt) {
    const int N = w->num_landmarks, M = w->num_observations;
    std::memset(S, 0, offsetof(Slot, x));
    r.N = N, r.M = M;
    S->N = N, S->M = M, S->NV = M - N;
    S->est_ex = w->estimate_extrinsic != 0, S->est_td = w->estimate_td != 0;
    S->max_iter = w->max_num_iterations;
    S->sharded = opt.sharded, S->pose_side = opt.pose_side;
    S->mail = (opt.slot == 0 && !opt.sharded && opt.mail && N <= MAIL_MAX_LM) ? opt.mail : 0;
    // (the loop's side of kernels_spec.h costs a store per pass and a compare-and-swap at its end; whether workers are started is
    // decided per call, enqueue_solve)
    S->spec_on = (opt.slot == 0 && opt.shadow && opt.marg_ahead && !opt.sharded && S->mail && N <= SPEC_MAX_LM) ? 1 : 0;
    S->mail_seq = opt.seq;
    for (int k = 0; k < 3; k++) S->g[k] = w->g[k];
    S->tr_over_row = w->row > 0.0 ? w->tr / w->row : 0.0;  // only the td factor reads it (row > 0: check_window)
    S->half_row = w->row / 2;
    S->sqrt_info = w->sqrt_info;
    S->fn_tol = opt.fn_tol;
    S->init_radius = opt.init_radius;
    std::memcpy(S->x0.pose, w->para_pose, sizeof S->x0.pose);
    std::memcpy(S->x0.sb, w->para_speed_bias, sizeof S->x0.sb);
    std::memcpy(S->x0.ex, w->para_ex_pose, sizeof S->x0.ex);
    S->x0.td = w->para_td;
    for (int i = 0; i < LFVIO_WINDOW_SIZE; i++) {
      S->imu[i] = w->imu[i];
      S->imu_active[i] = !(w->imu[i].sum_dt > 10.0);  // estimator.cpp:720
    }
    S->nLmBlocks = (N + LM_BLOCK - 1) / LM_BLOCK;
    // one part per landmark workgroup of k_lin, which forms it from its LDS tile: 64 landmarks, or 32 in the 8-lanes-per-track form
    S->lm_half = (N <= SPEC_MAX_LM && opt.lm_half) ? 1 : 0;
    S->schur_lm = S->lm_half ? SCHUR_LM / 2 : SCHUR_LM;
    S->nSchurParts = S->lm_half ? (N + SCHUR_LM / 2 - 1) / (SCHUR_LM / 2) : S->nLmBlocks;
    // (a little below the device's own threshold: a "yes" too many costs a few percent of one sweep, a "no" too many would put a
    // table with the residual chain's flavour in front of a kernel that does not look for it)
    auto off = [](const double *q) { return std::fabs((q[3] * q[3] + q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - 1.0) > 0.5 * TAB_OFF_SPHERE; };
    bool any = false;
    for (int f = 0; f < LFVIO_NUM_FRAMES; f++) any = any || off(w->para_pose[f] + 3);
    const bool ex = off(w->para_ex_pose + 3);
    r.offs_first = any || ex, r.offs_all = ex && !w->estimate_extrinsic;
  }

  // ---- landmarks: stable bucket sort by (start_frame, track length); the observations SoA, landmark-major in that order
  void landmarks(std::vector<int> &perm) {
    const int N = r.N;
    perm.resize(N);
    {
      int count[16 * 16 + 1] = {0};
      for (int l = 0; l < N; l++) count[w->start_frame[l] * 16 + (w->obs_offset[l + 1] - w->obs_offset[l]) + 1]++;
      for (int k = 0; k < 256; k++) count[k + 1] += count[k];
      for (int l = 0; l < N; l++) perm[count[w->start_frame[l] * 16 + (w->obs_offset[l + 1] - w->obs_offset[l])]++] = l;
    }
    int *lm_start = at<int>(L.lm_start), *lm_cnt = at<int>(L.lm_cnt), *lm_obs0 = at<int>(L.lm_obs0);
    int *lm_perm = at<int>(L.lm_perm), *lm_woff = at<int>(L.lm_woff);
    double *lam0 = at<double>(L.lam0);
    double *obs[8];
    for (int k = 0; k < 8; k++) obs[k] = at<double>(L.obs[k]);
    int o = 0;
    for (int dl = 0; dl < N; dl++) {
      const int l = perm[dl];
      const int s = w->start_frame[l], k = w->obs_offset[l + 1] - w->obs_offset[l], o0 = w->obs_offset[l];
      lm_start[dl] = s, lm_cnt[dl] = k, lm_obs0[dl] = o, lm_perm[dl] = l;
      lm_woff[dl] = dl == 0 ? 0 : lm_woff[dl - 1] + w_row_len(lm_cnt[dl - 1]);
      lam0[dl] = w->inv_depth[l];
      if (s == 0) r.N0++, r.kmax0 = std::max(r.kmax0, k);
      for (int q = 0; q < k; q++, o++) {
        const int src = o0 + q;
        obs[0][o] = w->obs_point[3 * src], obs[1][o] = w->obs_point[3 * src + 1], obs[2][o] = w->obs_point[3 * src + 2];
        obs[3][o] = w->obs_velocity[3 * src], obs[4][o] = w->obs_velocity[3 * src + 1], obs[5][o] = w->obs_velocity[3 * src + 2];
        obs[6][o] = w->obs_cur_td[src];
        obs[7][o] = w->obs_uv_y[src];
        if (q > 0) pair_count[s * 11 + s + q + 1]++;
      }
    }
    lm_woff[N] = N == 0 ? 0 : lm_woff[N - 1] + w_row_len(lm_cnt[N - 1]);
  }

  // ---- pair-major list of the non-anchor observations + chunk table
  const char *pairs_and_chunks() {
    for (int p = 0; p < NPAIR; p++) pair_count[p + 1] += pair_count[p];
    const int *lm_start = at<int>(L.lm_start), *lm_cnt = at<int>(L.lm_cnt), *lm_obs0 = at<int>(L.lm_obs0);
    int *pm_obs = at<int>(L.pm_obs), *pm_lm = at<int>(L.pm_lm);
    {
      int cursor[NPAIR];
      for (int p = 0; p < NPAIR; p++) cursor[p] = pair_count[p];
      for (int dl = 0; dl < r.N; dl++) {
        const int s = lm_start[dl], k = lm_cnt[dl];
        for (int q = 1; q < k; q++) {
          const int p = s * 11 + s + q;
          pm_obs[cursor[p]] = lm_obs0[dl] + q;
          pm_lm[cursor[p]] = dl;
          cursor[p]++;
        }
      }
    }
    int *chunk_pair = at<int>(L.chunk_pair), *chunk_begin = at<int>(L.chunk_begin), *chunk_end = at<int>(L.chunk_end);
    int nChunks = 0;
    for (int p = 0; p < NPAIR; p++) {
      S->pair_chunk0[p] = nChunks;
      for (int b = pair_count[p]; b < pair_count[p + 1]; b += CHUNK_MAX) {
        if (nChunks >= L.capChunks) return "chunk table overflow";
        chunk_pair[nChunks] = p, chunk_begin[nChunks] = b, chunk_end[nChunks] = std::min(b + CHUNK_MAX, pair_count[p + 1]);
        nChunks++;
      }
    }
    S->pair_chunk0[NPAIR] = nChunks;
    S->nChunks = r.nChunks = nChunks;
    return nullptr;
  }

  // ---- k_linw (kernels_linw.h): strips of <= 64 landmarks of one start frame, dealt to the four waves of the window's
  //      workgroup (all strips of a start frame on one wave: it is the one writer of that frame's pair blocks), and the
  //      observations once more in the orders its lanes read them — anchors by landmark, the others pair-major.
  //      k_linb: the same strips of a large single window as groups of one start frame, one workgroup each.
  void plans(bool want_linw, bool want_linb, int linb_max_groups) {
    r.linw = want_linw, r.linb = want_linb;
    if (!want_linw && !want_linb) return;
    LinwPlan &P = S->linw;
    const int N = r.N, *lm_start = at<int>(L.lm_start), *lm_cnt = at<int>(L.lm_cnt);
    int begin_s[LFVIO_NUM_FRAMES + 1];
    for (int s = 0, dl = 0; s <= LFVIO_NUM_FRAMES; s++) {
      while (dl < N && lm_start[dl] < s) dl++;
      begin_s[s] = dl;
    }
    for (int s = 0; s < LFVIO_NUM_FRAMES; s++) {
      int f = begin_s[s];  // (ascending track length inside a start frame)
      for (int o2 = 0; o2 < 12; o2++) {
        while (f < begin_s[s + 1] && lm_cnt[f] <= o2) f++;
        P.firstl[s][o2] = f;
      }
    }
    if (want_linb) groups(begin_s, linb_max_groups);
    else strips(begin_s);
    P.ok = (r.linw || r.linb) ? 1 : 0;
  }

  // the groups of k_linb: consecutive strips of one start frame sized by a cost model, the most expensive first (linb_plan.h)
  void groups(const int *begin_s, int max_groups) {
    LinwPlan &P = S->linw;
    const std::vector<LinbGroup> groups = linb_plan_groups(begin_s, LFVIO_NUM_FRAMES, at<int>(L.lm_cnt), LM_BLOCK, max_groups);
    int *g_lm0 = at<int>(L.linb_lm0), *g_ns = at<int>(L.linb_ns);
    r.linb_ng = (int)groups.size();
    if (r.linb_ng > L.capSchurParts) {  // (the partials live in the Schur partials' space)
      r.linb = false, r.linb_ng = 0;
      return;
    }
    for (int g = 0; g < r.linb_ng; g++) g_lm0[g] = groups[g].lm0, g_ns[g] = groups[g].n | (groups[g].s << 16);
    P.big = 1, P.ng = r.linb_ng, P.wt_ld = L.capLmBlocks * LM_BLOCK;
    for (int p = 0; p <= NPAIR; p++) P.pair_obs0[p] = pair_count[p];  // (the observations' copies are made on the device: k_linb_gather)
  }

  void strips(const int *begin_s) {
    LinwPlan &P = S->linw;
    const int *lm_cnt = at<int>(L.lm_cnt);
    struct Strip {
      int lm0, nlm, start, kmax;
    };
    std::vector<Strip> by_start[LFVIO_NUM_FRAMES];
    int cost[LFVIO_NUM_FRAMES] = {0}, n_strips = 0;
    for (int s = 0; s < LFVIO_NUM_FRAMES; s++)
      for (int l0 = begin_s[s]; l0 < begin_s[s + 1]; l0 += 64) {
        const int n = std::min(64, begin_s[s + 1] - l0);
        by_start[s].push_back(Strip{l0, n, s, lm_cnt[l0 + n - 1]});  // (ascending track length inside a start frame: the last one is the longest)
        cost[s] += lm_cnt[l0 + n - 1] - 1;
        n_strips++;
      }
    if (n_strips > LINW_MAX_STRIPS) {
      r.linw = false;
      return;
    }
    // longest-processing-time first over the start frames
    int order[LFVIO_NUM_FRAMES], load[LINW_WAVES] = {0};
    for (int s = 0; s < LFVIO_NUM_FRAMES; s++) order[s] = s;
    std::stable_sort(order, order + LFVIO_NUM_FRAMES, [&](int a, int b) { return cost[a] > cost[b]; });
    std::vector<Strip> per_wave[LINW_WAVES];
    for (int k = 0; k < LFVIO_NUM_FRAMES; k++) {
      const int s = order[k];
      if (by_start[s].empty()) continue;
      int wv = 0;
      for (int q = 1; q < LINW_WAVES; q++)
        if (load[q] < load[wv]) wv = q;
      load[wv] += cost[s];
      per_wave[wv].insert(per_wave[wv].end(), by_start[s].begin(), by_start[s].end());
    }
    int t = 0;
    for (int wv = 0; wv < LINW_WAVES; wv++) {
      P.wave_first[wv] = t;
      for (const Strip &st : per_wave[wv]) P.lm0[t] = (short)st.lm0, P.nlm[t] = (short)st.nlm, P.start[t] = (short)st.start, P.kmax[t] = (short)st.kmax, t++;
    }
    P.wave_first[LINW_WAVES] = t;
    P.n_strips = t;
    // the observations' second copies
    for (int p = 0; p <= NPAIR; p++) P.pair_obs0[p] = pair_count[p];
    const int *lm_obs0 = at<int>(L.lm_obs0), *pm_obs = at<int>(L.pm_obs);
    double *obs[8], *anc[8], *pmo[8];
    for (int k = 0; k < 8; k++) obs[k] = at<double>(L.obs[k]), anc[k] = at<double>(L.anc[k]), pmo[k] = at<double>(L.pmo[k]);
    for (int dl = 0; dl < r.N; dl++)
      for (int k = 0; k < 8; k++) anc[k][dl] = obs[k][lm_obs0[dl]];
    for (int q = 0; q < r.M - r.N; q++)
      for (int k = 0; k < 8; k++) pmo[k][q] = obs[k][pm_obs[q]];
    unsigned char *pm_pair = at<unsigned char>(L.pm_pair);
    for (int p = 0; p < NPAIR; p++)
      for (int q = pair_count[p]; q < pair_count[p + 1]; q++) pm_pair[q] = (unsigned char)p;
  }

  // Which (frame pair, local entry of its 20 x 20 block [Pi th_i Pj th_j tic th_ic td | r]) feed an H_pp / g_p entry is the same
  // for every window: a table built once per process.  Only the visual entries have a list (rows < KC: the packed prefix
  // [0, KC (KC + 1) / 2) and g_p[0, KC)); k_sum reads the bounds of the others but never uses them.
  struct PairLocal {
    short pair, local;
  };
  struct EntryTable {
    std::vector<int> first;  // [SUM_VIS + 1] into items
    std::vector<PairLocal> items;
  };
  static const EntryTable &entry_table() {
    static_assert(SUM_VIS_PACKED == KC * (KC + 1) / 2 && SUM_VIS == SUM_VIS_PACKED + KC, "compact gather index");
    static const EntryTable table = [] {
      auto col = [](int l, int i, int j) { return l < 6 ? 6 * i + l : l < 12 ? 6 * j + (l - 6) : l < 18 ? 66 + (l - 12) : 72; };
      EntryTable t;
      std::vector<std::vector<PairLocal>> per(SUM_VIS);
      for (int pp = 0; pp < NPAIR; pp++) {
        const int i = pp / 11, j = pp % 11;
        if (i >= j) continue;
        for (int lp = 0; lp < 19; lp++) {
          const int cp = col(lp, i, j);
          for (int lq = lp; lq < 20; lq++) {
            const int e = lq == 19 ? SUM_VIS_PACKED + cp : col(lq, i, j) * (col(lq, i, j) + 1) / 2 + cp;
            per[e].push_back(PairLocal{(short)pp, (short)(lp * 20 - (lp * (lp - 1)) / 2 + (lq - lp))});
          }
        }
      }
      t.first.assign(SUM_VIS + 1, 0);
      for (int e = 0; e < SUM_VIS; e++) {
        t.first[e + 1] = t.first[e] + (int)per[e].size();
        t.items.insert(t.items.end(), per[e].begin(), per[e].end());
      }
      return t;
    }();
    return table;
  }

  // ---- gather lists of k_sum: which Gram entries (chunk or, for large windows, frame pair; local index of the 20 x 20 block)
  //      add up to each packed H_pp / g_p entry.  Per upload the lists are ONE pass over the table's 2 774 entries — the pairs
  //      of the entry in ascending order, each with its chunks in ascending order: units ascend, so the marginalization's subset
  //      (pairs (0, j)) is a prefix of every list.
  //      The lists depend on nothing but pair_chunk0 and pre_gram (list_key): the ones the device holds from the last upload of
  //      the slot (list_items of them; -1: none) still stand if that has not changed — the pass over ~11 500 items is the largest
  //      single part of an upload.  A new key is stored here with list_items = -1; the caller sets list_items once the lists' copy
  //      is enqueued.
  const char *gather_lists(std::vector<int> &list_key, int &list_items, bool slot_uploaded) {
    S->pre_gram = r.nChunks > PRE_CHUNK_LIMIT ? 1 : 0;
    {
      std::vector<int> key(S->pair_chunk0, S->pair_chunk0 + NPAIR + 1);
      key.push_back(S->pre_gram);
      r.lists_cached = slot_uploaded && list_items >= 0 && key == list_key;
      if (!r.lists_cached) list_key.swap(key), list_items = -1;
    }
    if (r.lists_cached) {
      r.used_items = list_items;
      return nullptr;
    }
    const EntryTable &table = entry_table();
    int *sum_off = at<int>(L.sum_off), *sum_end_marg = at<int>(L.sum_end_marg), *sum_items = at<int>(L.sum_items);
    int n_items = 0;
    for (int e = 0; e < SUM_VIS; e++) {  // the bounds are stored by the compact index
      sum_off[e] = n_items;
      int marg_end = n_items;
      for (int k = table.first[e]; k < table.first[e + 1]; k++) {
        const int pp = table.items[k].pair, local = table.items[k].local;
        const int c0 = S->pair_chunk0[pp], c1 = S->pair_chunk0[pp + 1];
        if (c1 == c0) continue;
        if (n_items + (c1 - c0) > SUM_ITEMS_CAP) return "gather list overflow";
        if (S->pre_gram) {
          sum_items[n_items++] = pp * NGP + local;
        } else {
          for (int ch = c0; ch < c1; ch++) sum_items[n_items++] = ch * NGP + local;
        }
        if (pp < 11) marg_end = n_items;  // pairs (0, j): the marginalization's subset, a prefix of the list
      }
      sum_end_marg[e] = marg_end;
    }
    sum_off[SUM_VIS] = n_items;
    r.used_items = n_items;
    return nullptr;
  }

  // ---- the header's self-relative pointers to the input arrays
  void pointers() {
    S->lm_start.set(S, L.lm_start), S->lm_cnt.set(S, L.lm_cnt), S->lm_obs0.set(S, L.lm_obs0), S->lm_perm.set(S, L.lm_perm);
    S->lm_woff.set(S, L.lm_woff);
    S->lam0.set(S, L.lam0);
    for (int k = 0; k < 8; k++) S->obs[k].set(S, L.obs[k]);
    S->pm_obs.set(S, L.pm_obs), S->pm_lm.set(S, L.pm_lm);
    for (int k = 0; k < 8; k++) S->anc[k].set(S, L.anc[k]), S->pmo[k].set(S, L.pmo[k]);
    S->pm_pair.set(S, L.pm_pair);
    S->linb_lm0.set(S, L.linb_lm0), S->linb_ns.set(S, L.linb_ns);
    S->chunk_pair.set(S, L.chunk_pair), S->chunk_begin.set(S, L.chunk_begin), S->chunk_end.set(S, L.chunk_end);
    S->prior_J.set(S, L.prior_J), S->prior_r.set(S, L.prior_r);
    S->sum_off.set(S, L.sum_off), S->sum_end_marg.set(S, L.sum_end_marg), S->sum_items.set(S, L.sum_items);
  }
};

// Everything of the staging block `h` (Layout::linw_end bytes) that does not depend on the window's prior.  The window has passed
// check_window and fits the layout's capacity.  perm: device order -> caller order, built in the caller's vector.  list_key,
// list_items, slot_uploaded: the slot's gather-list cache (WindowPacker::gather_lists).  Returns nullptr, or the text of the error —
// the block is then half written, and a new list_key stands without lists.
inline const char *pack_window(const LfvioWindow *w, const Layout &L, char *h, const PackOptions &opt, std::vector<int> &perm, std::vector<int> &list_key,
                               int &list_items, bool slot_uploaded, PackResult *out) {
  *out = PackResult();
  WindowPacker p{w, L, h, (Slot *)h, *out};
  p.header(opt);
  p.landmarks(perm);
  if (const char *err = p.pairs_and_chunks()) return err;
  p.plans(opt.want_linw, opt.want_linb, opt.linb_max_groups);
  if (const char *err = p.gather_lists(list_key, list_items, slot_uploaded)) return err;
  p.pointers();
  return nullptr;
}

// The prior's section of the block packed by pack_window (whose result is r), and the two marginalization plans, which depend on it.
// pr: the window's input prior, checked (check_input_prior), or nullptr.  on_device (lfvio_batch_upload_chained_device): pr holds the
// structure only — the values (prior_x0, J, r) are copied on the device, k_prior_chain.  shard_kmax0 (sharded windows, >= 0): the
// longest track among the WHOLE window's frame-0 landmarks — the other ranks' shape the prior's blocks too (lfvio_shard_begin).
inline const char *pack_prior(const LfvioWindow *w, const LfvioPrior *pr, bool on_device, const Layout &L, char *h, const PackResult &r, int sharded,
                              int shard_kmax0) {
  Slot *S = (Slot *)h;
  for (int c = 0; c < KP; c++) S->prior_inv[c] = -1;
  if (pr) {
    S->prior_valid = 1, S->prior_n = pr->n, S->prior_nb = pr->num_blocks;
    for (int i = 0; i < pr->num_blocks; i++) {
      S->prior_kind[i] = pr->blocks[i].kind, S->prior_frame[i] = pr->blocks[i].frame, S->prior_idx[i] = pr->block_idx[i];
      if (!on_device) std::memcpy(S->prior_x0[i], pr->block_x0[i], sizeof(double) * 9);
      const int to = tangent_off(pr->blocks[i].kind, pr->blocks[i].frame);
      for (int e = 0; e < local_size(pr->blocks[i].kind); e++) {
        S->prior_cmap[pr->block_idx[i] + e] = to + e;
        S->prior_inv[to + e] = pr->block_idx[i] + e;
      }
    }
    if (!on_device) {
      std::memcpy(h + L.prior_J, pr->linearized_jacobians, sizeof(double) * pr->n * pr->n);
      std::memcpy(h + L.prior_r, pr->linearized_residuals, sizeof(double) * pr->n);
    }
  }
  const bool whole = sharded && shard_kmax0 >= 0;
  plan_marg(w, pr, LFVIO_MARGIN_OLD, r.N0, whole ? shard_kmax0 > 0 : r.N0 > 0, whole ? shard_kmax0 : r.kmax0, S->pair_chunk0[11], true, &S->marg[0]);
  plan_marg(w, pr, LFVIO_MARGIN_SECOND_NEW, 0, false, 0, 0, true, &S->marg[1]);
  for (int f = 0; f < 2; f++)
    if (S->marg[f].valid && (S->marg[f].n > 76 || S->marg[f].m15 + S->marg[f].n > 92))
      // k_marg_solve keeps the dense system in LDS: sized for what the reference's own marginalization produces
      // (10 poses + ex + td + one speed/bias = 76 kept, 15 dropped), not for an arbitrary hand-made prior
      return "prior keeps more than 76 tangent dimensions";
  return nullptr;
}
