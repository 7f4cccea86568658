"""lfvio_relative_pose (k_rp_hyp, k_rp_fit) against lfvio_two_view on every pair alone and against the numpy restatement
tests/relpose_ref.py.

  1  same bits as lfvio_two_view: for P = 1, 3, 10 over pairs of N in {21, 22, 30, 64, 65, 150, 1025 (one past TV_CHUNK), 4096 once}
     and S in {1, 7, 100}, each ungated pair's best_sample, best_score, num_inliers, mask, E, R_cand, t_cand equal Engine.two_view on
     that pair alone bit for bit, and good[] equals rint(front * N) reordered;
  2  against the restatement: gates, l, ok, good[] and chosen exact, average_parallax bit for bit, rotation (angle) and translation
     (angle between directions) in units of eps sigma_1/sigma_2 of the refit E_0 under test_two_view.loose_bar(N, "cand") — the
     project's bars, measured against the 50-digit fixtures.  The exact part holds under C1 - C3 of test_two_view on the restatement
     and gap >= 2 (the two largest good counts differ by at least 2); a pair that breaks that drops the exact comparisons only, at most
     10 % of the pairs;
  3  edges: all pairs gated, a slow pair in front of a good one, z == 0, garbage sample slots behind a small pair, a repeated call,
     every LFVIO_ERR_ARG case.

The device and the restatement may name the four candidates differently (lfvio_two_view does not pin which rotation is R1 or the sign
of t): good[] and chosen are compared through relpose_ref.match_candidates.
"""
import ctypes as C

import numpy as np
import pytest

import relpose_ref as rp
import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio import abi
from test_two_view import EPS, conditions, loose_bar

# (sizes of the pairs, S): P = 1, 3, 10; every N of the list, 4096 once; S = 1, 7, 100
CASES = {
    "P1_S100": ((150,), 100),
    "P3_S7": ((21, 64, 1025), 7),
    "P3_S1": ((4096, 30, 22), 1),
    "P10_S100": ((22, 30, 65, 150, 21, 64, 30, 22, 65, 150), 100),
    "P10_S7": ((20, 150, 1025, 64, 0, 65, 22, 21, 30, 19), 7),
}
_built = {}


def build(name):
    """The case's CSR, its sample sets and the restatement on it, computed once per session and left unchanged."""
    if name not in _built:
        sizes, S = CASES[name]
        k0 = 1000 * (sorted(CASES).index(name) + 1)
        cs = [gen.make_case(k0 + p, max(N, 1), noise_px=0.1, outliers=0.0 if N < 64 else 0.1, baseline=0.3 + 0.05 * p) for p, N in enumerate(sizes)]
        off = np.cumsum([0] + list(sizes)).astype(np.int32)
        bl = np.vstack([c["bl"][:N] for c, N in zip(cs, sizes)])
        br = np.vstack([c["br"][:N] for c, N in zip(cs, sizes)])
        sm = np.stack([gen.make_samples(k0 + 500 + p, max(N, 8), S, sort=True) for p, N in enumerate(sizes)]).astype(np.int32)
        for p, N in enumerate(sizes):
            if N <= 20:
                sm[p] = 0
        _built[name] = dict(off=off, bl=bl, br=br, sm=sm, ref=rp.relative_pose(off, bl, br, sm))
    return _built[name]


def pair_slice(c, p):
    a, b = int(c["off"][p]), int(c["off"][p + 1])
    return c["bl"][a:b], c["br"][a:b], c["sm"][p], slice(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_as_two_view(eng, name):
    c = build(name)
    d = eng.relative_pose(c["off"], c["bl"], c["br"], c["sm"])
    ran = 0
    for p, q in enumerate(d["pair"]):
        bl, br, sm, sl = pair_slice(c, p)
        assert q["num_matches"] == len(bl)
        if q["gate"] in (1, 2):
            continue
        t = eng.two_view(bl, br, sm)
        assert (q["gate"] == 3) == (t["status"] == 1), (name, p)
        assert (q["best_sample"], q["num_inliers"], q["best_score"]) == (t["best_sample"], t["num_inliers"], t["best_score"]), (name, p)
        if q["gate"] == 3:
            continue
        ran += 1
        for k in ("E", "R_cand", "t_cand"):
            assert q[k].tobytes() == t[k].tobytes(), (name, p, k)
        assert np.array_equal(d["mask"][sl], t["mask"]), (name, p)
        assert np.array_equal(q["good"], np.rint(t["front"] * len(bl)).astype(np.int32)[[0, 2, 1, 3]]), (name, p, q["good"], t["front"] * len(bl))
    assert ran >= 1


@pytest.mark.gpu
def test_against_the_restatement(eng):
    total, dropped, worst = 0, [], [0.0, 0.0]
    for name in sorted(CASES):
        c = build(name)
        ref = c["ref"]
        d = eng.relative_pose(c["off"], c["bl"], c["br"], c["sm"])
        print(name, "gates", [q["gate"] for q in d["pair"]], "l", d["l"])
        l_exact = True
        for p, (q, r) in enumerate(zip(d["pair"], ref["pair"])):
            tag = (name, p)
            N = r["num_matches"]
            assert q["num_matches"] == N and (q["gate"] in (1, 2)) == (r["gate"] in (1, 2)) and (q["gate"] == 1) == (r["gate"] == 1), tag
            assert np.array_equal(np.float64(q["average_parallax"]), np.float64(r["average_parallax"]), equal_nan=True), tag
            if r["gate"] in (1, 2):
                continue
            total += 1
            exact = r["gate"] == 0 and conditions(r) and r["gap"] >= 2
            if not exact:
                dropped.append(tag)
                l_exact = l_exact and (ref["l"] >= 0 and p > ref["l"])  # a pair behind l does not decide it
                if q["gate"] != 0 or r["gate"] != 0:
                    continue
            else:
                assert q["gate"] == 0 and q["best_sample"] == r["best_sample"] and q["num_inliers"] == r["num_inliers"], tag
            perm = rp.match_candidates(q, r)
            same = q["best_sample"] == r["best_sample"] and q["chosen"] == perm[r["chosen"]]
            if exact:
                assert np.array_equal(q["good"][perm], r["good"]), (tag, q["good"], perm, r["good"])
                assert same and q["inlier_cnt"] == r["inlier_cnt"] and q["ok"] == r["ok"], tag
            if exact or same:
                unit = EPS * r["rank2"]
                aR, aT = tv.rot_angle(q["rotation"], r["rotation"]) / unit, rp.direction_angle(q["translation"], r["translation"]) / unit
                print(f"  {tag} N={N} rotation {aR:.3g} translation {aT:.3g} (bar {loose_bar(N, 'cand'):.3g}) good {q['good'].tolist()} chosen {q['chosen']}")
                assert aR <= loose_bar(N, "cand") and aT <= loose_bar(N, "cand"), (tag, aR, aT)
                worst = [max(worst[0], aR), max(worst[1], aT)]
                assert np.array_equal(q["rotation"], q["rot"].T) and np.array_equal(q["rot"], q["R_cand"][q["chosen"] & 1]), tag
                assert np.array_equal(q["trans"], q["t_cand"] if q["chosen"] < 2 else -q["t_cand"]), tag
        if l_exact:
            assert d["l"] == ref["l"], name
            if d["l"] >= 0:
                assert np.array_equal(d["relative_R"], d["pair"][d["l"]]["rotation"]) and np.array_equal(d["relative_T"], d["pair"][d["l"]]["translation"])
    print(f"worst rotation {worst[0]:.3g}, translation {worst[1]:.3g} (eps sigma_1/sigma_2); dropped {dropped} of {total}")
    assert total >= 20 and len(dropped) <= 0.1 * total, dropped


def test_restatement_stays_within_the_cap():
    """CPU: on the cases above the restatement alone breaks C1 - C3 / gap >= 2 on at most 10 % of the pairs that run."""
    ran = [((n, p), r) for n in sorted(CASES) for p, r in enumerate(build(n)["ref"]["pair"]) if r["gate"] in (0, 3)]
    bad = [tag for tag, r in ran if not (r["gate"] == 0 and conditions(r) and r["gap"] >= 2)]
    print("pairs that run:", len(ran), "outside the conditions:", bad)
    assert len(ran) >= 20 and len(bad) <= 0.1 * len(ran)


# ---------------------------------------------------------------------------------------------------------------- edges
def marked_out():
    out = abi.RelativePoseOutC()
    out.l, out.pad_ = 77, 78
    for k in range(9):
        out.relative_R[k] = 1.5 + k
    for k in range(3):
        out.relative_T[k] = 20.5 + k
    for p in range(abi.WINDOW_SIZE):
        out.pair[p].gate, out.pair[p].chosen = 40 + p, 60 + p
    return out


def raw(eng, P, off, bl, br, S, sm, inlier, out):
    rin = abi.RelativePoseInC()
    rin.num_pairs, rin.num_samples = P, S
    ip = C.POINTER(C.c_int)
    dp = C.POINTER(C.c_double)
    rin.match_offset = off.ctypes.data_as(ip) if off is not None else None
    rin.bearing_l = bl.ctypes.data_as(dp) if bl is not None else None
    rin.bearing_r = br.ctypes.data_as(dp) if br is not None else None
    rin.samples = sm.ctypes.data_as(ip) if sm is not None else None
    return eng.lib.lfvio_relative_pose(eng.ctx, C.byref(rin), inlier.ctypes.data_as(C.POINTER(C.c_ubyte)) if inlier is not None else None,
                                       C.byref(out) if out is not None else None)


@pytest.mark.gpu
def test_edges(eng):
    c = build("P3_S7")
    good = gen.make_case(71, 40, noise_px=0.1, baseline=0.4)
    sm40 = gen.make_samples(72, 40, 7, sort=True)
    # all pairs gated: l = -1, LFVIO_OK, relative_R / T as the caller had them
    off = np.array([0, 20, 20, 60], np.int32)
    bl = np.vstack([good["bl"][:20], good["bl"]])
    br = np.vstack([good["br"][:20], good["bl"]])  # the third pair does not move
    sm = np.full((3, 7, 8), 10 ** 6, np.int32)  # garbage behind the small pairs: not an error
    sm[2] = sm40
    out, mask = marked_out(), np.full(60, 9, np.uint8)
    d = eng.relative_pose(off, bl, br, sm, out=out, inlier=mask)
    assert d["rc"] == 0 and d["l"] == -1 and [q["gate"] for q in d["pair"]] == [1, 1, 2] and np.all(mask == 9)
    assert np.array_equal(d["relative_R"].reshape(9), 1.5 + np.arange(9)) and np.array_equal(d["relative_T"], 20.5 + np.arange(3))
    assert out.pair[3].gate == 43 and out.pair[9].chosen == 69 and d["pair"][2]["average_parallax"] == 0.0 and d["pair"][0]["best_sample"] == -1
    # a slow pair in front of a good one
    br2 = np.vstack([good["br"][:20], good["bl"], good["br"]])
    bl2 = np.vstack([bl, good["bl"]])
    off2 = np.array([0, 20, 20, 60, 100], np.int32)
    sm2 = np.concatenate([sm, sm40[None]])
    d2 = eng.relative_pose(off2, bl2, br2, sm2)
    r2 = rp.relative_pose(off2, bl2, br2, sm2)
    assert [q["gate"] for q in d2["pair"]] == [1, 1, 2, 0] and d2["l"] == 3 == r2["l"] and d2["pair"][3]["ok"] == 1
    assert np.array_equal(d2["relative_R"], d2["pair"][3]["rotation"]) and np.array_equal(d2["relative_T"], d2["pair"][3]["translation"])
    assert np.array_equal(d2["mask"][60:], r2["pair"][3]["mask"]) and not d2["mask"][:60].any()
    # a repeated call: identical bits
    again = abi.RelativePoseOutC()
    first = abi.RelativePoseOutC()
    eng.relative_pose(off2, bl2, br2, sm2, out=first)
    eng.relative_pose(off2, bl2, br2, sm2, out=again)
    assert bytes(first) == bytes(again)
    # z == 0: in both frames of a match the term is inf - inf = NaN, NaN > 30 is false: gate 2
    zl, zr = good["bl"].copy(), good["br"].copy()
    zl[5], zr[5] = (0.6, 0.8, 0.0), (0.8, 0.6, 0.0)
    dz = eng.relative_pose([0, 40], zl, zr, sm40[None])
    assert dz["pair"][0]["gate"] == 2 and np.isnan(dz["pair"][0]["average_parallax"]) and dz["l"] == -1
    # (in one frame only: +inf, and inf * 160 > 30 is true, as in the reference: the pair runs)
    dz1 = eng.relative_pose([0, 40], zl, good["br"], sm40[None])
    assert dz1["pair"][0]["average_parallax"] == np.inf and dz1["pair"][0]["gate"] in (0, 3)


@pytest.mark.gpu
def test_argument_errors_leave_the_outputs_alone(eng):
    c = build("P3_S7")
    off, bl, br, sm = c["off"], c["bl"], c["br"], c["sm"]
    M = len(bl)
    out, mask = marked_out(), np.full(M, 9, np.uint8)
    before = bytes(out)
    bad_hi, bad_neg = sm.copy(), sm.copy()
    bad_hi[1, 3, 2] = 64  # pair 1 has 64 matches
    bad_neg[2, 0, 0] = -1
    big = np.array([0, 4097], np.int32)
    big_b = np.zeros((4097, 3))
    cases = [
        ("P = 0", (0, off, bl, br, 7, sm)), ("P = 11", (11, np.zeros(12, np.int32), bl, br, 7, np.zeros((11, 7, 8), np.int32))),
        ("S = 0", (3, off, bl, br, 0, sm)), ("S = 1025", (3, off, bl, br, 1025, np.zeros((3, 1025, 8), np.int32))),
        ("offset[0] != 0", (3, off + 1, bl, br, 7, sm)), ("descending", (3, np.array([0, 64, 21, M], np.int32), bl, br, 7, sm)),
        ("4097 matches", (1, big, big_b, big_b, 7, sm)), ("sample too large", (3, off, bl, br, 7, bad_hi)), ("sample negative", (3, off, bl, br, 7, bad_neg)),
        ("no offsets", (3, None, bl, br, 7, sm)), ("no bearing_l", (3, off, None, br, 7, sm)), ("no bearing_r", (3, off, bl, None, 7, sm)),
        ("no samples", (3, off, bl, br, 7, None)),
    ]
    for tag, (P, o, l, r, S, s) in cases:
        assert raw(eng, P, o, l, r, S, s, mask, out) == -1, tag  # LFVIO_ERR_ARG
        assert bytes(out) == before and np.all(mask == 9), tag
    assert raw(eng, 3, off, bl, br, 7, sm, mask, None) == -1 and np.all(mask == 9)
    assert eng.lib.lfvio_relative_pose(eng.ctx, None, mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(out)) == -1 and bytes(out) == before
    # the same arguments, valid: the call works, with and without a mask
    assert raw(eng, 3, off, bl, br, 7, sm, None, out) == 0 and out.pair[3].gate == 43 and out.l == c["ref"]["l"]
    assert raw(eng, 3, off, bl, br, 7, sm, mask, out) == 0
