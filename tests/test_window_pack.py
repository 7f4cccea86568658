"""CPU tests of the host packing of a window (lf-vio_amd/csrc/window_pack.h: pack_window, pack_prior, plan_marg) — where the device's data
layout is produced.  The header is plain C++, compiled here alone with g++ into a small shared object and driven through ctypes, like
tests/test_slot_args.py.  Everything asserted is integers or copied doubles: every comparison is exact equality against a numpy
restatement written here.

  (a) order: lm_perm is the stable sort of the caller's landmarks by (start_frame, track length); lm_start / lm_cnt / lm_obs0 / lm_woff /
      lam0 and the eight observation channels follow from it; N0 / kmax0 are frame 0's count and longest track;
  (b) pairs and chunks: pm_obs / pm_lm list every non-anchor observation once, by pair s * 11 + s + q ascending and in device landmark
      order inside a pair; the chunks of a pair tile its range in order, at most CHUNK_MAX each; the first 11 pair slots are the pairs (0, j);
  (c) gather lists, by their meaning: with a random small integer at every (unit, local index) of gram_part, the sums over
      sum_items[sum_off[e] : sum_off[e + 1]] are the visual part of packed H_pp and g_p assembled in numpy from the definition (the
      20 x 20 block of pair (i, j) has columns [Pi th_i | Pj th_j | tic th_ic | td | r]); units ascend in every list; the prefix up to
      sum_end_marg is the same assembly over the pairs (0, j) alone;
  (d) strips: every landmark in one strip of <= 64 of one start frame, kmax its longest track, all strips of a start frame on one wave,
      firstl, the second copies of the observations; 17 strips: no plan (the one thing the refused plan leaves in the block is the
      LinwPlan's firstl, which no kernel reads while ok == 0: everything outside Slot::linw is compared with the plan-less pack);
      the group plan at N = 321 (the groups themselves: tests/test_linb_plan.py);
  (e) the gather-list cache: the same pair table again is cached and leaves the lists' part of the block untouched;
  (f) prior_cmap / prior_inv and the two marginalization plans;
  (g) the header flags against the options.

"chunk table overflow" and "gather list overflow" cannot be reached with a layout made for the window (capChunks = 64 + M / CHUNK_MAX
is more than 55 pairs + (M - N) / CHUNK_MAX chunks; without pre_gram at most PRE_CHUNK_LIMIT chunks feed at most 209 items each, which is
SUM_ITEMS_CAP): they are not provoked here.  The size check of pack_prior is held at both sides of its bound by the sizes block
structures can reach: 76 kept columns pass, and 78 — ten poses and two speed/bias blocks, the smallest sum of 6s, 9s and one 1 above 76; no
structure keeps exactly 77 — are refused."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lfvio import abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "window_pack.h"
struct Field { const char *name; long long off, size; };
#define F(x) {#x, (long long)offsetof(T, x), (long long)sizeof(((T *)0)->x)},
#define T Slot
static const Field SLOT_FIELDS[] = {F(N) F(M) F(NV) F(nLmBlocks) F(nChunks) F(nSchurParts) F(est_ex) F(est_td) F(max_iter) F(prior_valid) F(prior_n) F(prior_nb)
  F(lm_half) F(schur_lm) F(sharded) F(pose_side) F(pre_gram) F(spec_on) F(mail_seq) F(mail) F(g) F(tr_over_row) F(half_row) F(sqrt_info) F(init_radius) F(fn_tol)
  F(x0) F(imu) F(imu_active) F(prior_kind) F(prior_frame) F(prior_idx) F(prior_x0) F(prior_cmap) F(prior_inv) F(pair_chunk0) F(marg) F(linw)
  F(lm_start) F(lm_cnt) F(lm_obs0) F(lm_perm) F(lm_woff) F(lam0) F(obs) F(pm_obs) F(pm_lm) F(anc) F(pmo) F(pm_pair) F(linb_lm0) F(linb_ns)
  F(chunk_pair) F(chunk_begin) F(chunk_end) F(prior_J) F(prior_r) F(sum_off) F(sum_end_marg) F(sum_items) F(x)};
#undef T
#define T LinwPlan
static const Field LINW_FIELDS[] = {F(ok) F(n_strips) F(wave_first) F(lm0) F(nlm) F(start) F(kmax) F(pair_obs0) F(firstl) F(big) F(ng) F(wt_ld)};
#undef T
#define T MargPlan
static const Field MARG_FIELDS[] = {F(valid) F(m15) F(n) F(nb) F(N0) F(nChunks0) F(use_imu0) F(use_visual) F(col) F(kind) F(frame) F(shifted_frame) F(idx)};
#undef T
template <int K>
static int fields(const Field (&t)[K], const char **name, long long *off, long long *size) {
  for (int k = 0; k < K; k++) name[k] = t[k].name, off[k] = t[k].off, size[k] = t[k].size;
  return K;
}
extern "C" int wp_fields(int which, const char **name, long long *off, long long *size) {
  return which == 0 ? fields(SLOT_FIELDS, name, off, size) : which == 1 ? fields(LINW_FIELDS, name, off, size) : fields(MARG_FIELDS, name, off, size);
}
extern "C" int wp_consts(const char **name, double *val) {
  int n = 0;
#define K(x) name[n] = #x, val[n++] = (double)(x);
  K(NPAIR) K(CHUNK_MAX) K(NGP) K(SUM_VIS_PACKED) K(SUM_VIS) K(SUM_ITEMS_CAP) K(PRE_CHUNK_LIMIT) K(LINW_MAX_STRIPS) K(LINW_WAVES) K(SPEC_MAX_LM) K(MAIL_MAX_LM)
  K(SCHUR_LM) K(LM_BLOCK) K(KP) K(KC) K(TAB_OFF_SPHERE) K(sizeof(MargPlan)) K(sizeof(LfvioPrior))
#undef K
  return n;
}
struct Handle {
  Layout L;
  std::vector<char> block;
  std::vector<int> perm, key;  // the caller's side of pack_window: lfvio_ctx::perm_build, SlotHostInfo::list_key / list_items / uploaded
  int items = -1;
  bool uploaded = false;
  PackResult r;
};
extern "C" void *wp_new(int maxN, int maxM) {
  Handle *h = new Handle;
  h->L = make_layout(maxN, maxM);
  h->block.assign(h->L.linw_end, 0);  // (the staging block of a context: Layout::linw_end bytes)
  return h;
}
extern "C" void wp_free(void *p) { delete (Handle *)p; }
extern "C" char *wp_block(void *p) { return ((Handle *)p)->block.data(); }
extern "C" int wp_layout(void *p, const char **name, long long *val) {
  const Layout &L = ((Handle *)p)->L;
  int n = 0;
#define G(x) name[n] = #x, val[n++] = (long long)L.x;
  G(maxN) G(maxM) G(capLmBlocks) G(capChunks) G(capSchurParts) G(in_begin) G(in_end) G(total) G(linw_begin) G(linw_end)
  G(lm_start) G(lm_cnt) G(lm_obs0) G(lm_perm) G(lm_woff) G(lam0) G(pm_obs) G(pm_lm) G(chunk_pair) G(chunk_begin) G(chunk_end)
  G(sum_off) G(sum_end_marg) G(sum_items) G(prior_J) G(prior_r) G(pm_pair) G(linb_lm0) G(linb_ns)
  G(obs[0]) G(obs[1]) G(obs[2]) G(obs[3]) G(obs[4]) G(obs[5]) G(obs[6]) G(obs[7])
  G(anc[0]) G(anc[1]) G(anc[2]) G(anc[3]) G(anc[4]) G(anc[5]) G(anc[6]) G(anc[7])
  G(pmo[0]) G(pmo[1]) G(pmo[2]) G(pmo[3]) G(pmo[4]) G(pmo[5]) G(pmo[6]) G(pmo[7])
#undef G
  return n;
}
// oi: slot sharded pose_side shadow marg_ahead lm_half want_linw want_linb linb_max_groups seq; od: fn_tol init_radius
// res: N M N0 kmax0 nChunks linw linb linb_ng used_items lists_cached offs_first offs_all
extern "C" const char *wp_pack(void *p, const LfvioWindow *w, const int *oi, long long mail, const double *od, int *res) {
  Handle *h = (Handle *)p;
  PackOptions o;
  o.slot = oi[0], o.sharded = oi[1], o.pose_side = oi[2], o.shadow = oi[3] != 0, o.marg_ahead = oi[4] != 0, o.lm_half = oi[5];
  o.want_linw = oi[6] != 0, o.want_linb = oi[7] != 0, o.linb_max_groups = oi[8], o.seq = oi[9];
  o.mail = mail, o.fn_tol = od[0], o.init_radius = od[1];
  const char *err = pack_window(w, h->L, h->block.data(), o, h->perm, h->key, h->items, h->uploaded, &h->r);
  const PackResult &r = h->r;
  const int out[12] = {r.N, r.M, r.N0, r.kmax0, r.nChunks, r.linw, r.linb, r.linb_ng, r.used_items, r.lists_cached, r.offs_first, r.offs_all};
  for (int k = 0; k < 12; k++) res[k] = out[k];
  return err;
}
extern "C" const char *wp_prior(void *p, const LfvioWindow *w, const LfvioPrior *pr, int on_device, int sharded, int shard_kmax0) {
  Handle *h = (Handle *)p;
  return pack_prior(w, pr, on_device != 0, h->L, h->block.data(), h->r, sharded, shard_kmax0);
}
extern "C" void wp_perm(void *p, int *out) {
  Handle *h = (Handle *)p;
  for (size_t k = 0; k < h->perm.size(); k++) out[k] = h->perm[k];
}
extern "C" int wp_cache_get(void *p, int *key, int *items) {
  Handle *h = (Handle *)p;
  for (size_t k = 0; k < h->key.size(); k++) key[k] = h->key[k];
  *items = h->items;
  return (int)h->key.size();
}
// what upload_window does once the lists' copy is enqueued: list_items = used_items, and the slot counts as uploaded
extern "C" void wp_cache_set(void *p, int uploaded, int items) {
  Handle *h = (Handle *)p;
  h->uploaded = uploaded != 0, h->items = items;
}
'''
RES = ("N", "M", "N0", "kmax0", "nChunks", "linw", "linb", "linb_ng", "used_items", "lists_cached", "offs_first", "offs_all")
POSE, SB, EX, TD = abi.BLOCK_POSE, abi.BLOCK_SPEEDBIAS, abi.BLOCK_EX_POSE, abi.BLOCK_TD
LOCAL = {POSE: 6, SB: 9, EX: 6, TD: 1}


def tangent_off(kind, frame):
    return {POSE: 6 * frame, SB: 73 + 9 * frame, EX: 66, TD: 72}[kind]


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="window_pack_")
    src, so = os.path.join(d, "wp.cpp"), os.path.join(d, "libwp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.wp_new.restype = C.c_void_p
    so.wp_block.restype = C.c_void_p
    so.wp_pack.restype = C.c_char_p
    so.wp_prior.restype = C.c_char_p
    so.wp_free.argtypes = so.wp_block.argtypes = [C.c_void_p]
    so.wp_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    so.wp_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    so.wp_prior.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    so.wp_perm.argtypes = [C.c_void_p, C.c_void_p]
    so.wp_cache_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    so.wp_cache_set.argtypes = [C.c_void_p, C.c_int, C.c_int]

    def table(which):
        name, off, size = (C.c_char_p * 80)(), (C.c_longlong * 80)(), (C.c_longlong * 80)()
        n = so.wp_fields(which, name, off, size)
        return {name[k].decode(): (off[k], size[k]) for k in range(n)}

    so.SLOT, so.LINW, so.MARG = table(0), table(1), table(2)
    name, val = (C.c_char_p * 32)(), (C.c_double * 32)()
    n = so.wp_consts(name, val)
    so.K = {name[k].decode(): (val[k] if name[k] == b"TAB_OFF_SPHERE" else int(val[k])) for k in range(n)}
    assert so.K["sizeof(LfvioPrior)"] == C.sizeof(abi.Prior)
    return so


class Pack:
    """One staging block with the host's side of its slot (permutation buffer, gather-list cache)."""

    def __init__(self, lib, maxN, maxM):
        self.lib, self.h = lib, lib.wp_new(maxN, maxM)
        name, val = (C.c_char_p * 64)(), (C.c_longlong * 64)()
        n = lib.wp_layout(self.h, name, val)
        self.L = {name[k].decode(): val[k] for k in range(n)}
        self.raw = (C.c_char * self.L["linw_end"]).from_address(lib.wp_block(self.h))
        self.bytes = np.frombuffer(self.raw, np.uint8)  # (a writable view of the block)

    def __del__(self):
        self.lib.wp_free(self.h)

    def arr(self, name, dtype, count):
        return np.frombuffer(self.raw, dtype, count, self.L[name])

    def hdr(self, name, dtype=np.int32, table=None, base=0):
        off, size = (table or self.lib.SLOT)[name]
        a = np.frombuffer(self.raw, dtype, size // np.dtype(dtype).itemsize, base + off)
        return a if a.size > 1 else a[0]

    def linw(self, name, dtype=np.int32):
        return self.hdr(name, dtype, self.lib.LINW, self.lib.SLOT["linw"][0])

    def marg(self, f, name):
        return self.hdr(name, np.int32, self.lib.MARG, self.lib.SLOT["marg"][0] + f * self.lib.K["sizeof(MargPlan)"])

    def pack(self, win, slot=0, sharded=0, pose_side=1, shadow=0, marg_ahead=0, lm_half=1, want_linw=0, want_linb=0, linb_max_groups=500, seq=1, mail=0,
             fn_tol=1e-6, init_radius=1e4):
        self.win, self.wc = win, win.c()
        oi = (C.c_int * 10)(slot, sharded, pose_side, shadow, marg_ahead, lm_half, want_linw, want_linb, linb_max_groups, seq)
        od, res = (C.c_double * 2)(fn_tol, init_radius), (C.c_int * 12)()
        err = self.lib.wp_pack(self.h, C.addressof(self.wc), oi, mail, od, res)
        self.res = dict(zip(RES, res))
        perm = np.zeros(max(win.N, 1), np.int32)
        self.lib.wp_perm(self.h, perm.ctypes.data)
        self.perm = perm[:win.N]
        return err

    def prior(self, pr, on_device=0, sharded=0, shard_kmax0=-1):
        self.pr = pr
        return self.lib.wp_prior(self.h, C.addressof(self.wc), C.addressof(pr) if pr is not None else None, on_device, sharded, shard_kmax0)

    def cache(self):
        key, items = (C.c_int * 200)(), C.c_int(0)
        n = self.lib.wp_cache_get(self.h, key, C.byref(items))
        return list(key[:n]), items.value


BASE = {}


def base_window():
    if "w" not in BASE:
        BASE["w"] = synth.make_window(0, 7)
    return BASE["w"]


def hand_window(start, cnt, seed=0, shuffle=True, **over):
    """The state and IMU of a small synthetic window around hand-made tracks; the packing only copies the observations' numbers."""
    rng = np.random.default_rng([seed, len(start)])
    start, cnt = np.asarray(start, np.int32), np.asarray(cnt, np.int32)
    if shuffle:
        order = rng.permutation(len(start))
        start, cnt = start[order], cnt[order]
    assert (cnt >= 2).all() and (start + cnt <= abi.NUM_FRAMES).all()
    M = int(cnt.sum())
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return base_window().copy(start_frame=start, obs_offset=off, inv_depth=rng.random(len(start)), obs_point=rng.random((M, 3)), obs_velocity=rng.random((M, 3)),
                              obs_cur_td=rng.random(M), obs_uv_y=rng.random(M), **over)


def classes(spec):
    start, cnt = [], []
    for s, k, n in spec:
        start += [s] * n
        cnt += [k] * n
    return start, cnt


def case_window(name):
    if name.startswith("plain"):
        n = int(name[5:])
        return synth.make_window(n + 1, n)
    if name == "pairs65_129":  # pair (0, 1) holds 65 observations, pair (3, 4) 129: chunks of 64 + 1 and 64 + 64 + 1
        return hand_window(*classes([(0, 2, 65), (3, 2, 129), (5, 4, 3), (9, 2, 2)]))
    if name == "classes16":  # sixteen (start frame, length) classes, 70 landmarks in one of them: two strips of start frame 2
        spec = [(0, 2, 3), (0, 5, 3), (0, 11, 3), (1, 3, 3), (1, 10, 3), (2, 4, 70), (2, 9, 3), (3, 2, 3), (4, 2, 3), (4, 7, 3), (5, 6, 3), (6, 3, 3), (7, 2, 3),
                (7, 4, 3), (8, 3, 3), (9, 2, 3)]
        return hand_window(*classes(spec))
    if name == "strips17":  # seven start frames of 65 landmarks (two strips each) and three of one: 17 strips
        return hand_window(*classes([(s, 2 + s % 3, 65) for s in range(7)] + [(s, 2, 1) for s in (7, 8, 9)]))
    if name == "pre_gram":  # 260 full-length tracks from every start frame: each of the 55 pairs has 5 chunks, 275 > PRE_CHUNK_LIMIT
        return hand_window(*classes([(s, 11 - s, 260) for s in range(10)]))
    raise KeyError(name)


PLAIN = ["plain%d" % n for n in (0, 1, 7, 64, 65, 300, 320, 321)]
HAND = ["pairs65_129", "classes16", "strips17", "pre_gram"]
STRIP_CASES = [c for c in PLAIN if c != "plain321"] + ["pairs65_129", "classes16"]
PACKED = {}


def packed(lib, name, plan=""):
    """The case's window packed once (plan: "", "linw" or "linb"), shared among the tests and left unchanged."""
    if (name, plan) not in PACKED:
        w = case_window(name)
        p = Pack(lib, w.N, w.M)
        assert p.pack(w, want_linw=plan == "linw", want_linb=plan == "linb") is None
        assert p.prior(None) is None
        PACKED[name, plan] = p
    return PACKED[name, plan]


def device_order(w):
    cnt = np.diff(w.obs_offset)
    return np.lexsort((cnt, w.start_frame)).astype(np.int32), cnt  # (stable: by start frame, then track length, then the caller's order)


def pair_table(start, cnt, obs0):
    """Non-anchor observations by pair, in device landmark order inside a pair: (pair, observation, landmark) columns."""
    dl = np.repeat(np.arange(len(start)), cnt - 1)
    q = np.concatenate([np.arange(1, k) for k in cnt]) if len(cnt) else np.zeros(0, np.int64)
    pair = start[dl] * 11 + start[dl] + q
    o = np.argsort(pair, kind="stable")
    return pair[o].astype(np.int64), (obs0[dl] + q)[o].astype(np.int32), dl[o].astype(np.int32)


@pytest.mark.parametrize("case", PLAIN + HAND)
def test_order_of_landmarks_and_observations(lib, case):
    p = packed(lib, case)
    w, N, M = p.win, p.win.N, p.win.M
    perm, cnt = device_order(w)
    assert (p.res["N"], p.res["M"]) == (N, M) and (p.hdr("N"), p.hdr("M"), p.hdr("NV")) == (N, M, M - N)
    assert np.array_equal(p.perm, perm) and np.array_equal(p.arr("lm_perm", np.int32, N), perm)
    lm_cnt = cnt[perm]
    assert np.array_equal(p.arr("lm_start", np.int32, N), w.start_frame[perm]) and np.array_equal(p.arr("lm_cnt", np.int32, N), lm_cnt)
    assert np.array_equal(p.arr("lm_obs0", np.int32, N), np.concatenate([[0], np.cumsum(lm_cnt)])[:N])
    assert np.array_equal(p.arr("lm_woff", np.int32, N + 1), np.concatenate([[0], np.cumsum(6 * lm_cnt + 9)]))
    assert np.array_equal(p.arr("lam0", np.float64, N), w.inv_depth[perm])
    src = np.concatenate([np.arange(w.obs_offset[l], w.obs_offset[l + 1]) for l in perm]) if N else np.zeros(0, np.int64)
    want = [w.obs_point[src, 0], w.obs_point[src, 1], w.obs_point[src, 2], w.obs_velocity[src, 0], w.obs_velocity[src, 1], w.obs_velocity[src, 2],
            w.obs_cur_td[src], w.obs_uv_y[src]]
    for k in range(8):
        assert np.array_equal(p.arr("obs[%d]" % k, np.float64, M), want[k]), k
    first = w.start_frame == 0
    assert p.res["N0"] == int(first.sum()) and p.res["kmax0"] == (int(cnt[first].max()) if first.any() else 0)
    # the header's self-relative pointers lead to the layout's arrays
    for name in ("lm_start", "lm_cnt", "lm_obs0", "lm_perm", "lm_woff", "lam0", "pm_obs", "pm_lm", "pm_pair", "linb_lm0", "linb_ns", "chunk_pair", "chunk_begin",
                 "chunk_end", "prior_J", "prior_r", "sum_off", "sum_end_marg", "sum_items"):
        assert lib.SLOT[name][0] + int(p.hdr(name, np.int64)) == p.L[name], name
    for name in ("obs", "anc", "pmo"):
        for k in range(8):
            assert lib.SLOT[name][0] + 8 * k + int(p.hdr(name, np.int64)[k]) == p.L["%s[%d]" % (name, k)], (name, k)


@pytest.mark.parametrize("case", PLAIN + HAND)
def test_pairs_and_chunks(lib, case):
    p, K = packed(lib, case), lib.K
    N, M, NPAIR, CH = p.win.N, p.win.M, K["NPAIR"], K["CHUNK_MAX"]
    start, cnt, obs0 = (p.arr(n, np.int32, N) for n in ("lm_start", "lm_cnt", "lm_obs0"))
    pair, pm_obs, pm_lm = pair_table(start, cnt, obs0)
    assert np.array_equal(p.arr("pm_obs", np.int32, M - N), pm_obs) and np.array_equal(p.arr("pm_lm", np.int32, M - N), pm_lm)
    anchors = set(obs0.tolist())
    assert sorted(pm_obs.tolist()) == [o for o in range(M) if o not in anchors]  # every non-anchor observation exactly once
    begin = np.searchsorted(pair, np.arange(NPAIR + 1))  # first pair-major observation of every pair
    pc0, nCh = p.hdr("pair_chunk0"), p.res["nChunks"]
    assert len(pc0) == NPAIR + 1 and (np.diff(pc0) >= 0).all() and pc0[0] == 0 and pc0[NPAIR] == nCh == p.hdr("nChunks")
    c_pair, c_begin, c_end = (p.arr(n, np.int32, nCh) for n in ("chunk_pair", "chunk_begin", "chunk_end"))
    for q in range(NPAIR):
        ch = slice(pc0[q], pc0[q + 1])
        n_obs = begin[q + 1] - begin[q]
        assert pc0[q + 1] - pc0[q] == (n_obs + CH - 1) // CH
        assert (c_pair[ch] == q).all()
        assert np.array_equal(c_begin[ch], begin[q] + CH * np.arange(pc0[q + 1] - pc0[q]))
        assert np.array_equal(c_end[ch], np.minimum(c_begin[ch] + CH, begin[q + 1]))
    if case == "pairs65_129":
        assert pc0[2] - pc0[1] == 2 and pc0[3 * 11 + 4 + 1] - pc0[3 * 11 + 4] == 3
        assert (c_end - c_begin)[pc0[1]:pc0[2]].tolist() == [64, 1] and (c_end - c_begin)[pc0[37]:pc0[38]].tolist() == [64, 64, 1]
    # the first 11 pair slots are the pairs (0, j): exactly the non-anchor observations of the landmarks anchored at frame 0
    assert (start[pm_lm[:begin[11]]] == 0).all() and (start[pm_lm[begin[11]:]] > 0).all()
    assert p.marg(0, "nChunks0") == pc0[11] and p.marg(0, "N0") == p.res["N0"]


def gather_assembly(K, unit_pair, G, only_first=False):
    """The visual part of packed H_pp and g_p, [SUM_VIS], from the definition: unit u of frame pair (i, j) holds the upper triangle of the
    20 x 20 block over the columns [Pi th_i | Pj th_j | tic th_ic | td | r]; local index of (lp <= lq): lp * 20 - lp (lp - 1) / 2 + lq - lp."""
    out = np.zeros(K["SUM_VIS"], np.int64)
    lp, lq = np.triu_indices(20)
    local = lp * 20 - (lp * (lp - 1)) // 2 + (lq - lp)
    keep = lp < 19  # (19, 19) is the cost: no entry of H_pp or g_p
    lp, lq, local = lp[keep], lq[keep], local[keep]
    for u, pp in enumerate(unit_pair):
        i, j = divmod(int(pp), 11)
        if only_first and i != 0:
            continue
        cols = np.array([6 * i + k for k in range(6)] + [6 * j + k for k in range(6)] + [66 + k for k in range(6)] + [72])
        cp = cols[lp]
        cq = cols[np.minimum(lq, 18)]
        e = np.where(lq == 19, K["SUM_VIS_PACKED"] + cp, cq * (cq + 1) // 2 + cp)  # packed lower triangle, row cq >= column cp | g_p[cp]
        np.add.at(out, e, G[u, local])
    return out


@pytest.mark.parametrize("case", PLAIN + HAND)
def test_gather_lists_add_up_to_the_assembly(lib, case):
    p, K = packed(lib, case), lib.K
    NGP, VIS, nCh = K["NGP"], K["SUM_VIS"], p.res["nChunks"]
    pre = int(p.hdr("pre_gram"))
    assert pre == (1 if nCh > K["PRE_CHUNK_LIMIT"] else 0) and pre == (case == "pre_gram")
    unit_pair = np.arange(K["NPAIR"]) if pre else p.arr("chunk_pair", np.int32, nCh)
    if pre:  # (a pair without observations has no unit's worth of data: it must not appear in any list)
        pc0 = p.hdr("pair_chunk0")
        unit_live = np.diff(pc0) > 0
    else:
        unit_live = np.ones(len(unit_pair), bool)
    rng = np.random.default_rng(7)
    G = rng.integers(-50, 50, size=(max(len(unit_pair), 1), NGP)).astype(np.int64)
    used = p.res["used_items"]
    assert not p.res["lists_cached"] and 0 <= used <= K["SUM_ITEMS_CAP"]
    off, end_marg, items = p.arr("sum_off", np.int32, VIS + 1), p.arr("sum_end_marg", np.int32, VIS), p.arr("sum_items", np.int32, used)
    assert off[0] == 0 and off[VIS] == used and (np.diff(off) >= 0).all() and (off[:-1] <= end_marg).all() and (end_marg <= off[1:]).all()
    unit = items // NGP
    assert (unit < len(unit_pair)).all() and unit_live[unit].all() if used else True
    inner = np.ones(max(used - 1, 0), bool)
    inner[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < used)] - 1] = False  # (positions where the next list begins)
    assert (np.diff(unit)[inner] > 0).all()  # units ascend inside every list
    csum = np.concatenate([[0], np.cumsum(G.reshape(-1)[items])])
    Gl = G * unit_live[:len(G), None] if len(unit_pair) else G
    assert np.array_equal(csum[off[1:]] - csum[off[:-1]], gather_assembly(K, unit_pair, Gl))
    assert np.array_equal(csum[end_marg] - csum[off[:-1]], gather_assembly(K, unit_pair, Gl, only_first=True))


@pytest.mark.parametrize("case", STRIP_CASES)
def test_strips(lib, case):
    p, K = packed(lib, case, "linw"), lib.K
    N, M = p.win.N, p.win.M
    assert p.res["linw"] and not p.res["linb"] and p.linw("ok") == 1 and p.linw("big") == 0
    start, cnt, obs0 = (p.arr(n, np.int32, N) for n in ("lm_start", "lm_cnt", "lm_obs0"))
    ns, wf = int(p.linw("n_strips")), p.linw("wave_first")
    assert ns <= K["LINW_MAX_STRIPS"] and wf[0] == 0 and (np.diff(wf) >= 0).all() and wf[K["LINW_WAVES"]] == ns
    lm0, nlm, st, kmax = (p.linw(n, np.int16)[:ns] for n in ("lm0", "nlm", "start", "kmax"))
    seen, wave_of = np.zeros(N, np.int32), {}
    for t in range(ns):
        own = slice(lm0[t], lm0[t] + nlm[t])
        assert 1 <= nlm[t] <= 64 and (start[own] == st[t]).all() and kmax[t] == cnt[own].max()
        seen[own] += 1
        wave_of.setdefault(int(st[t]), set()).add(int(np.searchsorted(wf, t, side="right") - 1))
    assert (seen == 1).all() and all(len(v) == 1 for v in wave_of.values())
    if case == "classes16":
        assert sorted(nlm[st == 2].tolist()) == [9, 64] and ns == 11
    firstl = p.linw("firstl").reshape(abi.NUM_FRAMES, 12)
    begin = np.searchsorted(start, np.arange(abi.NUM_FRAMES + 1))
    for s in range(abi.NUM_FRAMES):
        for o in range(12):
            assert firstl[s, o] == begin[s] + int((cnt[begin[s]:begin[s + 1]] <= o).sum()), (s, o)
    pair, pm_obs, _ = pair_table(start, cnt, obs0)
    pair_obs0 = p.linw("pair_obs0")
    assert np.array_equal(pair_obs0, np.searchsorted(pair, np.arange(K["NPAIR"] + 1)))
    assert np.array_equal(p.arr("pm_pair", np.uint8, M - N), pair.astype(np.uint8))
    for k in range(8):
        obs = p.arr("obs[%d]" % k, np.float64, M)
        assert np.array_equal(p.arr("anc[%d]" % k, np.float64, N), obs[obs0]) and np.array_equal(p.arr("pmo[%d]" % k, np.float64, M - N), obs[pm_obs])
    # the plan changes nothing outside Slot::linw and its own arrays
    q = packed(lib, case)
    lo, hi = lib.SLOT["linw"][0], lib.SLOT["linw"][0] + lib.SLOT["linw"][1]
    assert np.array_equal(p.bytes[:lo], q.bytes[:lo]) and np.array_equal(p.bytes[hi:p.L["linw_begin"]], q.bytes[hi:p.L["linw_begin"]])


def test_seventeen_strips_leave_no_plan(lib):
    p, q = packed(lib, "strips17", "linw"), packed(lib, "strips17")
    assert not p.res["linw"] and not p.res["linb"] and p.linw("ok") == 0 and p.linw("n_strips") == 0
    lo, hi = lib.SLOT["linw"][0], lib.SLOT["linw"][0] + lib.SLOT["linw"][1]
    assert np.array_equal(p.bytes[:lo], q.bytes[:lo]) and np.array_equal(p.bytes[hi:], q.bytes[hi:])
    assert {k: v for k, v in p.res.items()} == {k: v for k, v in q.res.items()}


def test_group_plan_at_321(lib):
    p, q, K = packed(lib, "plain321", "linb"), packed(lib, "plain321"), lib.K
    N = p.win.N
    assert p.res["linb"] and not p.res["linw"] and p.linw("ok") == 1 and p.linw("big") == 1 and p.linw("n_strips") == 0
    ng = p.res["linb_ng"]
    assert 0 < ng <= p.L["capSchurParts"] and p.linw("ng") == ng and p.linw("wt_ld") == p.L["capLmBlocks"] * K["LM_BLOCK"]
    start, cnt, obs0 = (p.arr(n, np.int32, N) for n in ("lm_start", "lm_cnt", "lm_obs0"))
    g_lm0, g_ns = p.arr("linb_lm0", np.int32, ng), p.arr("linb_ns", np.int32, ng)
    seen = np.zeros(N, np.int32)
    for a, word in zip(g_lm0, g_ns):
        n, s = word & 0xffff, word >> 16
        assert 1 <= n <= 512 and (start[a:a + n] == s).all()
        seen[a:a + n] += 1
    assert (seen == 1).all()
    pair, _, _ = pair_table(start, cnt, obs0)
    assert np.array_equal(p.linw("pair_obs0"), np.searchsorted(pair, np.arange(K["NPAIR"] + 1)))
    lo, hi = lib.SLOT["linw"][0], lib.SLOT["linw"][0] + lib.SLOT["linw"][1]
    assert np.array_equal(p.bytes[:lo], q.bytes[:lo]) and np.array_equal(p.bytes[hi:p.L["linw_begin"]], q.bytes[hi:p.L["linw_begin"]])


def test_gather_list_cache(lib):
    K = lib.K
    w1, w2 = case_window("plain300"), case_window("pairs65_129")
    p = Pack(lib, max(w1.N, w2.N), max(w1.M, w2.M))
    lists = slice(p.L["sum_off"], p.L["sum_items"] + 4 * K["SUM_ITEMS_CAP"])
    assert p.pack(w1) is None and not p.res["lists_cached"]
    used = p.res["used_items"]
    first_lists = np.concatenate([p.arr("sum_off", np.int32, K["SUM_VIS"] + 1), p.arr("sum_end_marg", np.int32, K["SUM_VIS"]), p.arr("sum_items", np.int32, used)])
    key, items = p.cache()
    assert key == p.hdr("pair_chunk0").tolist() + [int(p.hdr("pre_gram"))] and items == -1  # the key stands, the lists are not on the device yet
    # a pack whose copies never went out (refused on the way): the same window again is NOT cached
    assert p.pack(w1) is None and not p.res["lists_cached"] and p.cache()[1] == -1
    p.lib.wp_cache_set(p.h, 1, used)  # the copies are enqueued
    p.bytes[lists] = 0xA5
    assert p.pack(w1) is None and p.res["lists_cached"] and p.res["used_items"] == used
    assert (p.bytes[lists] == 0xA5).all()  # sum_off / sum_end_marg / sum_items untouched ...
    assert p.L["sum_off"] < p.L["sum_end_marg"] < p.L["sum_items"] and p.L["prior_r"] < p.L["sum_off"]  # ... so the caller's copy ends at L.sum_off: all other inputs lie in front
    assert p.cache() == (key, used)
    # another pair table: not cached, the key is replaced and the lists are written again
    assert p.pack(w2) is None and not p.res["lists_cached"]
    key2, items2 = p.cache()
    assert key2 != key and key2 == p.hdr("pair_chunk0").tolist() + [0] and items2 == -1
    assert not (p.bytes[p.L["sum_off"]:p.L["sum_off"] + 4 * K["SUM_VIS"]] == 0xA5).all()
    p.lib.wp_cache_set(p.h, 1, p.res["used_items"])
    # a slot that has never been uploaded holds no lists, whatever the key says
    p.lib.wp_cache_set(p.h, 0, p.res["used_items"])
    assert p.pack(w2) is None and not p.res["lists_cached"]
    # back to the first window: its lists are the ones of the first pack
    p.lib.wp_cache_set(p.h, 1, p.res["used_items"])
    assert p.pack(w1) is None and not p.res["lists_cached"] and p.res["used_items"] == used
    again = np.concatenate([p.arr("sum_off", np.int32, K["SUM_VIS"] + 1), p.arr("sum_end_marg", np.int32, K["SUM_VIS"]), p.arr("sum_items", np.int32, used)])
    assert np.array_equal(again, first_lists)


def make_prior(blocks, seed=1):
    rng = np.random.default_rng(seed)
    pr = abi.Prior()
    pr.valid, pr.m, pr.num_blocks = 1, 15, len(blocks)
    pos = 0
    for i, (k, f) in enumerate(blocks):
        pr.blocks[i].kind, pr.blocks[i].frame, pr.block_idx[i] = k, f, pos
        pos += LOCAL[k]
        for e in range(9):
            pr.block_x0[i][e] = rng.random()
    pr.n = pos
    J, r = rng.random(pos * pos), rng.random(pos)
    C.memmove(pr.linearized_jacobians, J.ctypes.data, 8 * pos * pos)
    C.memmove(pr.linearized_residuals, r.ctypes.data, 8 * pos)
    return pr, J, r


def with_sum_dt(win, sum_dt):
    imu = list(win.imu)
    imu[0] = abi.Preintegration.from_buffer_copy(bytes(imu[0]))
    imu[0].sum_dt = sum_dt
    return win.copy(imu=imu)


def expected_plan(win, blocks, flag, any0, kmax0):
    """(dropped, kept) blocks of MarginalizationInfo in canonical order (kind, then frame), or None where there is nothing to do."""
    present, dropped = set(blocks or ()), set()
    if flag == abi.MARGIN_OLD:
        dropped |= {(k, f) for k, f in present if k in (POSE, SB) and f == 0}
        if win.imu[0].sum_dt < 10.0:
            present |= {(POSE, 0), (SB, 0), (POSE, 1), (SB, 1)}
            dropped |= {(POSE, 0), (SB, 0)}
        if any0:
            present |= {(POSE, j) for j in range(kmax0)} | {(EX, 0)} | ({(TD, 0)} if win.estimate_td else set())
            dropped |= {(POSE, 0)}
    else:
        if (POSE, abi.WINDOW_SIZE - 1) not in present:
            return None
        dropped = {(POSE, abi.WINDOW_SIZE - 1)}
    return sorted(dropped), sorted(present - dropped)


def check_plan(p, f, win, blocks, any0=None, kmax0=None):
    flag = (abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW)[f]
    any0 = p.res["N0"] > 0 if any0 is None else any0
    want = expected_plan(win, blocks, flag, any0, p.res["kmax0"] if kmax0 is None else kmax0)
    if want is None:
        assert p.marg(f, "valid") == 0
        return None
    dropped, kept = want
    m15, n, nb = int(p.marg(f, "m15")), int(p.marg(f, "n")), int(p.marg(f, "nb"))
    assert p.marg(f, "valid") == 1 and m15 == sum(LOCAL[k] for k, _ in dropped) and n == sum(LOCAL[k] for k, _ in kept) and nb == len(kept)
    col = p.marg(f, "col")
    here = col >= 0
    assert sorted(col[here].tolist()) == list(range(m15 + n))  # a bijection of the present columns onto [0, m15 + n)
    want_col, pos = np.full(lib_KP, -1), 0
    for k, fr in dropped + kept:  # the dropped blocks first
        want_col[tangent_off(k, fr):tangent_off(k, fr) + LOCAL[k]] = np.arange(pos, pos + LOCAL[k])
        pos += LOCAL[k]
    assert np.array_equal(col, want_col)
    kind, frame, shifted, idx = (p.marg(f, name)[:nb] for name in ("kind", "frame", "shifted_frame", "idx"))
    assert list(zip(kind.tolist(), frame.tolist())) == kept
    for b, (k, fr) in enumerate(kept):
        assert col[tangent_off(k, fr)] == m15 + idx[b]
        framed = k in (POSE, SB)
        assert shifted[b] == (fr if not framed else fr - 1 if flag == abi.MARGIN_OLD else (abi.WINDOW_SIZE - 1 if fr == abi.WINDOW_SIZE else fr))
    return m15, n, nb


lib_KP = abi.KP
STD_BLOCKS = [(POSE, f) for f in range(10)] + [(SB, 0), (EX, 0), (TD, 0)]  # what a MARGIN_OLD step leaves: 76 rows


@pytest.mark.parametrize("on_device", (0, 1))
def test_prior_section(lib, on_device):
    w = case_window("plain65")
    p = Pack(lib, w.N, w.M)
    pr, J, r = make_prior(STD_BLOCKS)
    assert p.pack(w) is None
    p.bytes[p.L["prior_J"]:p.L["prior_J"] + 8 * pr.n * pr.n] = 0xA5
    p.bytes[p.L["prior_r"]:p.L["prior_r"] + 8 * pr.n] = 0xA5
    x0_off, x0_size = lib.SLOT["prior_x0"]
    p.bytes[x0_off:x0_off + x0_size] = 0xA5
    assert p.prior(pr, on_device=on_device) is None
    nb = len(STD_BLOCKS)
    assert (p.hdr("prior_valid"), p.hdr("prior_n"), p.hdr("prior_nb")) == (1, 76, nb)
    assert list(zip(p.hdr("prior_kind")[:nb].tolist(), p.hdr("prior_frame")[:nb].tolist())) == STD_BLOCKS
    assert p.hdr("prior_idx")[:nb].tolist() == [pr.block_idx[i] for i in range(nb)]
    cmap, inv = p.hdr("prior_cmap"), p.hdr("prior_inv")
    want_inv = np.full(abi.KP, -1)
    for i, (k, f) in enumerate(STD_BLOCKS):
        want_inv[tangent_off(k, f):tangent_off(k, f) + LOCAL[k]] = pr.block_idx[i] + np.arange(LOCAL[k])
    assert np.array_equal(inv, want_inv)  # -1 outside the prior's columns
    cols = np.flatnonzero(inv >= 0)
    assert len(cols) == pr.n and np.array_equal(cmap[inv[cols]], cols) and np.array_equal(inv[cmap[:pr.n]], np.arange(pr.n))  # mutually inverse
    x0 = p.hdr("prior_x0", np.float64).reshape(-1, 9)
    Jb, rb = p.arr("prior_J", np.float64, pr.n * pr.n), p.arr("prior_r", np.float64, pr.n)
    if on_device:  # the values are the device's: k_prior_chain writes them
        assert (p.bytes[x0_off:x0_off + x0_size] == 0xA5).all() and (Jb.view(np.uint8) == 0xA5).all() and (rb.view(np.uint8) == 0xA5).all()
    else:
        assert np.array_equal(x0[:nb], np.array([pr.x0(i) for i in range(nb)])) and np.array_equal(Jb, J) and np.array_equal(rb, r)
    for f in range(2):
        check_plan(p, f, w, STD_BLOCKS)
    # without a prior
    assert p.pack(w) is None and p.prior(None) is None
    assert p.hdr("prior_valid") == 0 and (p.hdr("prior_inv") == -1).all()
    check_plan(p, 0, w, None)
    assert p.marg(1, "valid") == 0  # MARGIN_SECOND_NEW without a prior: nothing to do


def test_marginalization_plans(lib):
    # a frame-0 track over all 11 frames, a short first IMU interval, td estimated, no prior: 15 dropped, 76 kept in 13 blocks
    w = hand_window(*classes([(0, 11, 1), (0, 3, 4), (2, 5, 6)]), estimate_td=1)
    assert w.imu[0].sum_dt < 10.0
    p = Pack(lib, w.N, w.M)
    assert p.pack(w) is None and p.prior(None) is None
    assert check_plan(p, 0, w, None) == (15, 76, 13)
    assert (p.marg(0, "use_imu0"), p.marg(0, "use_visual"), p.marg(0, "N0")) == (1, 1, 5) and p.marg(1, "valid") == 0
    # the first IMU interval too long to be a factor (sum_dt >= 10): only the pose of frame 0 is dropped, 6 x 6
    wl = with_sum_dt(w, 10.0)
    assert p.pack(wl) is None and p.prior(None) is None
    m15, n, nb = check_plan(p, 0, wl, None)
    assert m15 == 6 and (n, nb) == (67, 12) and p.marg(0, "use_imu0") == 0
    # MARGIN_SECOND_NEW: a prior without the pose of frame 9 passes through, one with it drops those 6 columns
    no9 = [(POSE, f) for f in range(9)] + [(SB, 0), (EX, 0)]
    pr, _, _ = make_prior(no9)
    assert p.pack(w) is None and p.prior(pr) is None
    assert p.marg(1, "valid") == 0 and check_plan(p, 1, w, no9) is None
    check_plan(p, 0, w, no9)
    pr, _, _ = make_prior(STD_BLOCKS)
    assert p.prior(pr) is None and check_plan(p, 1, w, STD_BLOCKS) == (6, 70, 12)
    # a rank's share of a sharded window: the block structure is the whole window's (its longest frame-0 track), the sweep the rank's own
    ws = hand_window(*classes([(0, 3, 4), (2, 5, 6)]))
    assert p.pack(ws, sharded=1) is None and p.prior(None, sharded=1, shard_kmax0=7) is None
    check_plan(p, 0, ws, None, any0=True, kmax0=7)
    assert p.marg(0, "N0") == 4
    wn = hand_window(*classes([(2, 5, 6)]))
    newest = [(POSE, 10), (POSE, 9), (SB, 10), (TD, 0)]  # frame 10 becomes 9
    pr10, _, _ = make_prior(newest)
    assert p.pack(wn) is None and p.prior(pr10) is None and check_plan(p, 1, wn, newest) == (6, 16, 3)
    check_plan(p, 0, wn, newest)
    assert p.pack(wn, sharded=1) is None and p.prior(None, sharded=1, shard_kmax0=0) is None
    check_plan(p, 0, wn, None, any0=False, kmax0=0)
    assert p.pack(wn, sharded=1) is None and p.prior(None, sharded=1, shard_kmax0=4) is None
    check_plan(p, 0, wn, None, any0=True, kmax0=4)
    assert p.marg(0, "N0") == 0 and p.marg(0, "use_visual") == 0


def test_prior_size_bound(lib):
    w = hand_window(*classes([(2, 5, 6)]))  # no landmark at frame 0: the poses come from the prior
    p = Pack(lib, w.N, w.M)
    assert p.pack(w) is None
    # 76 kept (what the reference's own marginalization produces) passes ...
    pr, _, _ = make_prior([(POSE, f) for f in range(2, 11)] + [(EX, 0), (TD, 0)])  # + pose 1, sb 1 of the IMU factor: 60 + 9 + 6 + 1
    assert p.prior(pr) is None and check_plan(p, 0, w, [(POSE, f) for f in range(2, 11)] + [(EX, 0), (TD, 0)])[1] == 76
    # ... the next size a block structure can have does not: ten poses and two speed/bias blocks, 78
    blocks = [(POSE, f) for f in range(2, 11)] + [(SB, 2)]
    pr, _, _ = make_prior(blocks)
    assert p.prior(pr) == b"prior keeps more than 76 tangent dimensions"
    assert int(p.marg(0, "n")) == 78
    # m15 + n > 92 with n <= 76 cannot be reached by MARGIN_OLD (m15 <= 15) — the second condition guards the LDS size on its own


def quat_off(q, half_tol):
    return abs((q[3] * q[3] + q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - 1.0) > half_tol


def test_off_sphere_flags(lib):
    half = 0.5 * lib.K["TAB_OFF_SPHERE"]
    w = case_window("plain7")
    p = Pack(lib, w.N, w.M)
    assert p.pack(w) is None
    want_any = any(quat_off(w.pose[f, 3:], half) for f in range(abi.NUM_FRAMES)) or quat_off(w.ex_pose[3:], half)
    assert bool(p.res["offs_first"]) == want_any
    unit = np.array([0.0, 0.0, 0.0, 1.0])
    on = w.copy(pose=np.hstack([w.pose[:, :3], np.tile(unit, (abi.NUM_FRAMES, 1))]), ex_pose=np.concatenate([w.ex_pose[:3], unit]))
    assert p.pack(on) is None and (p.res["offs_first"], p.res["offs_all"]) == (0, 0)
    for eps, off in ((1e-15, False), (2e-15, False), (4e-15, True), (1e-14, True), (-1e-14, True)):
        q = np.array([0.0, 0.0, 0.0, 1.0 + eps])
        assert quat_off(q, half) == off, eps  # (|q|^2 - 1 is about 2 eps against half the device's 1e-14)
        for f in (0, 5, 10):
            pose = on.pose.copy()
            pose[f, 3:] = q
            assert p.pack(on.copy(pose=pose)) is None and (p.res["offs_first"], p.res["offs_all"]) == (int(off), 0), (eps, f)
        ex = np.concatenate([on.ex_pose[:3], q])
        assert p.pack(on.copy(ex_pose=ex, estimate_extrinsic=1)) is None and (p.res["offs_first"], p.res["offs_all"]) == (int(off), 0)
        assert p.pack(on.copy(ex_pose=ex, estimate_extrinsic=0)) is None and (p.res["offs_first"], p.res["offs_all"]) == (int(off), int(off))


@pytest.mark.parametrize("n", (320, 321))
def test_header_follows_the_options(lib, n):
    K = lib.K
    w = hand_window(*classes([(s, 3, n // 8 + (1 if s < n % 8 else 0)) for s in range(8)]), estimate_extrinsic=0, tr=0.03)
    assert w.N == n
    p = Pack(lib, w.N, w.M)
    MAILBOX = 0x7F1234567000
    for slot, sharded, shadow, ahead, lm_half, mail in itertools.product((0, 1), (0, 2), (0, 1), (0, 1), (0, 1), (0, MAILBOX)):
        assert p.pack(w, slot=slot, sharded=sharded, pose_side=2 if sharded else 1, shadow=shadow, marg_ahead=ahead, lm_half=lm_half, mail=mail, seq=41 + slot,
                      fn_tol=1e-7, init_radius=3e3) is None
        want_mail = mail if (slot == 0 and not sharded and n <= K["MAIL_MAX_LM"]) else 0
        assert int(p.hdr("mail", np.int64)) == want_mail
        assert p.hdr("spec_on") == int(slot == 0 and shadow and ahead and not sharded and want_mail != 0 and n <= K["SPEC_MAX_LM"])
        half = int(n <= K["SPEC_MAX_LM"] and lm_half)
        blocks = (n + K["LM_BLOCK"] - 1) // K["LM_BLOCK"]
        assert (p.hdr("lm_half"), p.hdr("schur_lm"), p.hdr("nLmBlocks")) == (half, K["SCHUR_LM"] // 2 if half else K["SCHUR_LM"], blocks)
        assert p.hdr("nSchurParts") == ((n + K["SCHUR_LM"] // 2 - 1) // (K["SCHUR_LM"] // 2) if half else blocks)
        assert (p.hdr("sharded"), p.hdr("pose_side"), p.hdr("mail_seq")) == (sharded, 2 if sharded else 1, 41 + slot)
    assert (p.hdr("fn_tol", np.float64), p.hdr("init_radius", np.float64)) == (1e-7, 3e3)
    assert (p.hdr("est_ex"), p.hdr("est_td"), p.hdr("max_iter")) == (0, w.estimate_td, w.max_num_iterations)
    assert p.hdr("g", np.float64).tolist() == list(w.g) and p.hdr("sqrt_info", np.float64) == w.sqrt_info
    assert p.hdr("tr_over_row", np.float64) == w.tr / w.row and p.hdr("half_row", np.float64) == w.row / 2
    x0 = p.hdr("x0", np.float64)
    assert np.array_equal(x0, np.concatenate([w.pose.ravel(), w.speed_bias.ravel(), w.ex_pose, [w.td]]))
    assert bytes(p.hdr("imu", np.uint8)) == b"".join(bytes(i) for i in w.imu)
    assert p.hdr("imu_active").tolist() == [int(not (i.sum_dt > 10.0)) for i in w.imu]
    late = with_sum_dt(w, 10.5)
    assert p.pack(late) is None and p.hdr("imu_active").tolist() == [0] + [1] * (abi.WINDOW_SIZE - 1)
