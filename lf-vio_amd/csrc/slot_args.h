// slot_args.h — where the arrays of a slot blob lie (Layout, by capacity) and the byte offsets k_lin and k_spec_begin take as
// a kernel ARGUMENT (SlotArgs).  Plain C++ (no HIP): lfvio_hip.hip builds both per context, tests/test_slot_args.py compiles this
// file alone and walks the capacities on the CPU.
//
// Why arguments: inside the blob the arrays are addressed through the self-relative offsets (GP<T>) of the slot header, so a kernel's
// first data loads cannot leave until the header's scalar loads have come back — one dependent memory round trip (1 - 1.5 us) of a
// kernel that runs for 5 - 20.  An offset that arrives with the launch lets the first loads of the data leave together with the
// header's.  Such a load is issued before the header has said how large the window is, so it is SPECULATIVE: its index is clamped into
// the array's capacity (the cap_* members, never less than one entry), and what it brings is dropped where the header then says the
// index was past the window.  slot_arg_spans() states, per offset, how far the kernels' first-round loads can reach.
#pragma once
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#include <algorithm>
#include <cstddef>
#include "dev_types.h"

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Layout {  // byte offsets inside one slot blob, by capacity
  int maxN = 0, maxM = 0;
  int capLmBlocks = 0, capChunks = 0, capSchurParts = 0;
  size_t in_begin = 0, in_end = 0, total = 0;
  size_t anc[8], pmo[8], pm_pair, linb_lm0, linb_ns, linw_begin = 0, linw_end = 0;  // k_linw's copies of the observations (behind the regular inputs: uploaded on their own, resident batches only)
  size_t lm_start, lm_cnt, lm_obs0, lm_perm, lm_woff, lam0, obs[8], pm_obs, pm_lm, chunk_pair, chunk_begin, chunk_end, sum_off, sum_end_marg, sum_items, prior_J,
      prior_r;
  size_t lam[2], lamE[SPEC_EXTRA], cost_partE, prior_A, a, b, W, Wt, scale_l, grad_l, gn_l, diag_l, einv_l, d1, d2, gram_part, pairG, schur_part,
      xch, lm_part, cost_part, imu_out, imu_raw, mscr, eig_aux;
};

inline Layout make_layout(int maxN, int maxM) {
  Layout L;
  L.maxN = maxN;
  L.maxM = maxM;
  L.capLmBlocks = std::max(1, (maxN + LM_BLOCK - 1) / LM_BLOCK);
  L.capChunks = 64 + maxM / CHUNK_MAX;
  // (one part per landmark workgroup of k_lin: 64 landmarks each, or 32 for windows of at most SPEC_MAX_LM landmarks — Slot::lm_half)
  L.capSchurParts = std::max(L.capLmBlocks + 1, 2 * ((std::min(maxN, SPEC_MAX_LM) + LM_BLOCK - 1) / LM_BLOCK));
  static_assert(LINB_LEN >= SCHUR_LEN, "the Schur partials of k_lin share the array of k_linb's group partials, which are the larger");
  size_t o = align_up(sizeof(Slot), 256);
  auto take = [&](size_t bytes) {
    size_t r = o;
    o = align_up(o + bytes, 256);
    return r;
  };
  const size_t N = std::max(maxN, 1), M = std::max(maxM, 1), LB = (size_t)L.capLmBlocks * LM_BLOCK;
  L.in_begin = o;
  L.lm_start = take(N * 4), L.lm_cnt = take(N * 4), L.lm_obs0 = take(N * 4), L.lm_perm = take(N * 4);
  L.lm_woff = take((N + 1) * 4);
  L.lam0 = take(N * 8);
  for (int k = 0; k < 8; k++) L.obs[k] = take(M * 8);
  L.pm_obs = take(M * 4), L.pm_lm = take(M * 4);
  L.chunk_pair = take((size_t)L.capChunks * 4), L.chunk_begin = take((size_t)L.capChunks * 4),
  L.chunk_end = take((size_t)L.capChunks * 4);
  // (the two arrays whose used part varies most come last, so that an upload copies [in_begin, used end of sum_items)
  // and the n x n the prior really has — 0.2 MB instead of 0.7 MB at 300 landmarks)
  L.prior_r = take(LFVIO_MAX_PRIOR_DIM * 8);
  L.sum_off = take((size_t)(SUM_VIS + 1) * 4), L.sum_end_marg = take((size_t)SUM_VIS * 4);
  L.sum_items = take((size_t)SUM_ITEMS_CAP * 4);
  L.prior_J = take((size_t)LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM * 8);
  L.in_end = o;
  L.linw_begin = o;
  for (int k = 0; k < 8; k++) L.anc[k] = take(N * 8);
  for (int k = 0; k < 8; k++) L.pmo[k] = take(M * 8);
  L.pm_pair = take(M);
  L.linb_lm0 = take(((size_t)L.capLmBlocks + LFVIO_NUM_FRAMES + 1) * 4), L.linb_ns = take(((size_t)L.capLmBlocks + LFVIO_NUM_FRAMES + 1) * 4);  // (at most a group per strip)
  L.linw_end = o;
  L.lam[0] = take(LB * 8), L.lam[1] = take(LB * 8);
  for (int k = 0; k < SPEC_EXTRA; k++) L.lamE[k] = take((size_t)SPEC_MAX_LM * 8);
  L.cost_partE = take((size_t)SPEC_EXTRA * (SPEC_MAX_LM / 64) * LMS * 8);
  L.prior_A = take((size_t)LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM * 8);
  L.a = take(LB * 8), L.b = take(LB * 8), L.W = take(LB * WLD * 8);
  L.Wt = take((size_t)WT_PAIRS * std::max((size_t)SPEC_MAX_LM, LB) * 16);  // (a large window's rows are LB apart: k_linb)
  L.scale_l = take(LB * 8), L.grad_l = take(LB * 8), L.gn_l = take(LB * 8), L.diag_l = take(LB * 8);
  L.einv_l = take(LB * 8), L.d1 = take(LB * 8), L.d2 = take(LB * 8);
  L.gram_part = take((size_t)L.capChunks * NGP * 8);
  L.pairG = take((size_t)NPAIR * NGP * 8);
  L.schur_part = take((size_t)L.capSchurParts * LINB_LEN * 8);  // (k_linb's partials live there too: LINB_LEN > SCHUR_LEN doubles per group, at most a group per strip)
  L.xch = take((size_t)XCH_ALLOC * 8);
  L.lm_part = take((size_t)L.capLmBlocks * LMS * 8);
  L.cost_part = take((size_t)L.capLmBlocks * LMS * 8);
  L.imu_out = take((size_t)LFVIO_WINDOW_SIZE * IMU_OUT * 8);
  L.imu_raw = take((size_t)LFVIO_WINDOW_SIZE * IMU_RAW * 8);
  L.mscr = take((size_t)HPP_CAP * 8);
  L.eig_aux = take(4096);
  L.total = align_up(o, 4096);
  return L;
}

// Byte offsets from the Slot a kernel runs on, the same for every slot of a context; passed BY VALUE to k_lin and k_spec_begin.  The
// first group are INPUT arrays: in a worker's shadow slot (kernels_spec.h) they lead back into slot 0, like the shadow's copies of the
// header's GP members do (`back`: the shadow's distance from slot 0).
struct SlotArgs {
  long long lm_start, lm_cnt, lm_obs0, lm_woff;     // [cap_lm_in] ints ([cap_lm_in + 1]: lm_woff)
  long long obs0, obs_stride;                       // the eight observation channels, obs_stride bytes apart
  long long pm_obs, pm_lm;                          // pair-major observation and landmark indices
  long long chunk_pair, chunk_begin, chunk_end;     // [cap_chunks] ints
  long long prior_J;                                // LFVIO_MAX_PRIOR_DIM^2 doubles
  // work arrays: the slot's own
  long long lam[2];                                 // [cap_lm] doubles
  long long cost_part, cost_partE;                  // [cap_blocks][LMS] | [SPEC_EXTRA][SPEC_MAX_LM / 64][LMS]
  int cap_lm_in, cap_chunks, cap_blocks, cap_lm;
};
constexpr int SLOT_INPUT_OFFSETS = 12;  // the leading long long members that are input arrays

// The index of every SPECULATIVE load, as the kernels form it (i >= 0; a capacity is never less than one entry).  slot_arg_spans()
// below derives each array's reach from these same functions, so a clamp against the wrong capacity shows in tests/test_slot_args.py.
__host__ __device__ inline int first_clamp(int i, int cap) { return i < cap ? i : cap - 1; }
__host__ __device__ inline int first_lm_in_index(const SlotArgs &A, int l) { return first_clamp(l, A.cap_lm_in); }   // lm_start / lm_cnt / lm_obs0 / lm_woff (k_lin's landmark role)
__host__ __device__ inline int first_chunk_index(const SlotArgs &A, int c) { return first_clamp(c, A.cap_chunks); }  // chunk_* (k_lin's Gram role)
__host__ __device__ inline int first_lm_index(const SlotArgs &A, int l) { return first_clamp(l, A.cap_lm); }         // lam[cur] (k_spec_begin)
__host__ __device__ inline int first_block_index(int cap_blocks, int lane) { return first_clamp(lane, cap_blocks); }  // cost_part: a block per lane (decide_first)
__host__ __device__ inline int first_blockE_index(int cap_blocks, int lane) { return first_clamp(lane, cap_blocks < SPEC_MAX_LM / 64 ? cap_blocks : SPEC_MAX_LM / 64); }  // cost_partE, per candidate
constexpr int FIRST_PRIOR_J = ((76 * 76 + 255) / 256) * 256;  // k_lin's prior role: J0 of up to 76 rows, a whole number of rounds of 256 threads, whatever the prior's size
static_assert(FIRST_PRIOR_J <= LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM, "the speculative rounds of J0 stay inside the array");

inline SlotArgs slot_args(const Layout &L, size_t back = 0) {
  SlotArgs A;
  const long long bk = (long long)back;
  A.lm_start = (long long)L.lm_start - bk, A.lm_cnt = (long long)L.lm_cnt - bk, A.lm_obs0 = (long long)L.lm_obs0 - bk, A.lm_woff = (long long)L.lm_woff - bk;
  A.obs0 = (long long)L.obs[0] - bk, A.obs_stride = (long long)(L.obs[1] - L.obs[0]);
  A.pm_obs = (long long)L.pm_obs - bk, A.pm_lm = (long long)L.pm_lm - bk;
  A.chunk_pair = (long long)L.chunk_pair - bk, A.chunk_begin = (long long)L.chunk_begin - bk, A.chunk_end = (long long)L.chunk_end - bk;
  A.prior_J = (long long)L.prior_J - bk;
  A.lam[0] = (long long)L.lam[0], A.lam[1] = (long long)L.lam[1];
  A.cost_part = (long long)L.cost_part, A.cost_partE = (long long)L.cost_partE;
  A.cap_lm_in = std::max(L.maxN, 1), A.cap_chunks = L.capChunks, A.cap_blocks = L.capLmBlocks, A.cap_lm = L.capLmBlocks * LM_BLOCK;
  return A;
}

// Per offset of SlotArgs: `bytes` — what, from the offset on, a first-round (speculative, clamped) load of the kernels can touch, from
// the index functions above at the largest index there is (at least the array's first entry: the arrays behind pm_* and obs0 are
// addressed from indices other arrays hold, never speculatively); `array` — the bytes Layout gave the array.  `input`: the offset
// leads into slot 0 in a shadow slot's variant.
struct SlotArgSpan {
  const char *name;
  long long off, bytes, array;
  int input;
};
constexpr int SLOT_ARG_SPANS = 15;  // entries slot_arg_spans() writes
inline int slot_arg_spans(const Layout &L, const SlotArgs &A, SlotArgSpan *out) {
  int n = 0;
  auto put = [&](const char *name, long long off, long long bytes, long long array, int input) { out[n++] = SlotArgSpan{name, off, bytes, array, input}; };
  constexpr int BIG = 0x7fffffff;
  const long long N = std::max(L.maxN, 1), M = std::max(L.maxM, 1), LB = (long long)L.capLmBlocks * LM_BLOCK;
  const long long lin = (first_lm_in_index(A, BIG) + 1) * 4ll, ch = (first_chunk_index(A, BIG) + 1) * 4ll;
  put("lm_start", A.lm_start, lin, N * 4, 1), put("lm_cnt", A.lm_cnt, lin, N * 4, 1), put("lm_obs0", A.lm_obs0, lin, N * 4, 1);
  put("lm_woff", A.lm_woff, lin, (N + 1) * 4, 1);
  put("obs0", A.obs0, 7 * A.obs_stride + 8, 7 * A.obs_stride + M * 8, 1);  // (all eight channels from obs0)
  put("pm_obs", A.pm_obs, 4, M * 4, 1), put("pm_lm", A.pm_lm, 4, M * 4, 1);
  put("chunk_pair", A.chunk_pair, ch, (long long)L.capChunks * 4, 1), put("chunk_begin", A.chunk_begin, ch, (long long)L.capChunks * 4, 1);
  put("chunk_end", A.chunk_end, ch, (long long)L.capChunks * 4, 1);
  put("prior_J", A.prior_J, (long long)FIRST_PRIOR_J * 8, (long long)LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM * 8, 1);
  put("lam0", A.lam[0], (first_lm_index(A, BIG) + 1) * 8ll, LB * 8, 0), put("lam1", A.lam[1], (first_lm_index(A, BIG) + 1) * 8ll, LB * 8, 0);
  put("cost_part", A.cost_part, (first_block_index(A.cap_blocks, BIG) + 1ll) * LMS * 8, (long long)L.capLmBlocks * LMS * 8, 0);
  put("cost_partE", A.cost_partE, ((long long)(SPEC_EXTRA - 1) * (SPEC_MAX_LM / 64) + first_blockE_index(A.cap_blocks, BIG) + 1) * LMS * 8,
      (long long)SPEC_EXTRA * (SPEC_MAX_LM / 64) * LMS * 8, 0);
  return n;
}
