"""CPU: the numpy restatement of relativePose() (tests/relpose_ref.py) on synthetic two-view geometry, and the host mirror's
WindowEstimator::relativePose() without a device.

The restatement is what tests/test_relative_pose.py holds lfvio_relative_pose to, so it is held to the truth here: on noisy
two-view cases (rays through z <= 0 included: the 40 - 120 degree annulus of the fixtures' generator) its rotation / translation meet
the true relative pose; every one of recoverPose's four candidate slots wins somewhere; the >= chain of solve_5pts.cpp:507-534 on
hand-made ties; the gates at N = 20 / 21 and on a pair that does not move; l skips gated and failed pairs.
"""
import numpy as np

import relpose_ref as rp
import twoview_ref as tv
from golden import gen_twoview_hp as gen
from lfvio import abi

W = abi.WINDOW_SIZE


def csr(cases):
    off = np.cumsum([0] + [len(c["bl"]) for c in cases]).astype(np.int32)
    return off, np.vstack([c["bl"] for c in cases]), np.vstack([c["br"] for c in cases])


def test_restatement_meets_the_true_pose_and_every_slot_wins():
    """X_r = R X_l + t: the newest camera's rotation in frame l is R^T and its position -R^T t (direction only: unit norm).
    Bars from the geometry, not from the code: bearings carry sigma = 0.1 px / f radians of noise; one point at depth d seen over a
    baseline b fixes the direction of t to about sigma d / b, so with d <= 12 and b >= 0.5 the worst single point gives 24 sigma.  Sixty
    points average that down, the coupling of rotation and translation pushes it up: the bars are 10 x the single-point figures,
    rotation 10 sigma and direction 240 sigma."""
    sigma = 0.1 / gen.FOCAL
    slots, worst, behind = set(), [0.0, 0.0], 0
    for seed in range(40):
        c = gen.make_case(300 + seed, 60, noise_px=0.1, baseline=0.5 + 0.01 * seed)
        r = rp.solve_pair(c["bl"], c["br"], gen.make_samples(400 + seed, 60, 30))
        assert r["gate"] == 0 and r["ok"] == 1 and r["inlier_cnt"] == r["good"][r["chosen"]] == r["good"].max(), seed
        behind += int((c["bl"][:, 2] <= 0).sum() + (c["br"][:, 2] <= 0).sum())
        dR = tv.rot_angle(r["rotation"], c["R"].T)
        dT = rp.direction_angle(r["translation"], -c["R"].T @ c["t"])
        assert abs(np.linalg.norm(r["translation"]) - 1.0) < 1e-12 and np.array_equal(r["rotation"], r["rot"].T)
        assert dR < 10 * sigma and dT < 240 * sigma, (seed, dR, dT)
        worst = [max(worst[0], dR), max(worst[1], dT)]
        slots.add(r["chosen"])
    print(f"worst rotation {worst[0]:.2e} rad, direction {worst[1]:.2e} rad; slots that won: {sorted(slots)}")
    assert slots == {0, 1, 2, 3} and behind > 100  # (a third of the annulus lies at z <= 0)


def test_the_chain_on_ties():
    for good, want in (((5, 5, 5, 5), 0), ((4, 5, 5, 5), 1), ((4, 4, 5, 5), 2), ((1, 2, 3, 4), 3), ((3, 5, 5, 4), 1), ((5, 3, 5, 1), 0),
                       ((0, 0, 0, 0), 0), ((2, 3, 1, 3), 1), ((2, 1, 3, 3), 2), ((7, 0, 0, 8), 3)):
        assert rp.choose(good) == want, good


def test_recover_pose_counts_all_matches_in_its_own_order():
    """good[] is over ALL matches (no mask), in the order (R1,t) (R2,t) (R1,-t) (R2,-t): two_view's front[] reordered."""
    c = gen.make_case(7, 80, noise_px=0.3, outliers=0.2)
    r = tv.two_view(c["bl"], c["br"], gen.make_samples(8, 80, 50))
    good, chosen = rp.recover_pose(c["bl"], c["br"], r["R_cand"][0], r["R_cand"][1], r["t_cand"])
    assert np.array_equal(good, np.rint(r["front"] * 80).astype(int)[[0, 2, 1, 3]]) and good.sum() <= 2 * 80 and good[chosen] == good.max()


def test_gates():
    c = gen.make_case(11, 21, noise_px=0.1, baseline=0.5)
    s = gen.make_samples(12, 20, 20)
    r20 = rp.solve_pair(c["bl"][:20], c["br"][:20], s)
    assert r20["gate"] == 1 and r20["num_matches"] == 20 and r20["best_sample"] == -1 and r20["chosen"] == -1 and r20["ok"] == 0
    r21 = rp.solve_pair(c["bl"], c["br"], s)
    assert r21["gate"] == 0 and r21["num_matches"] == 21 and r21["average_parallax"] * 160 > 30
    still = rp.solve_pair(c["bl"], c["bl"], s)  # the camera did not move: parallax 0
    assert still["gate"] == 2 and still["average_parallax"] == 0.0
    zl, zr = c["bl"].copy(), c["br"].copy()
    zl[5], zr[5] = (0.6, 0.8, 0.0), (0.8, 0.6, 0.0)  # z == 0 in both frames: inf - inf = NaN, and NaN > 30 is false
    rz = rp.solve_pair(zl, zr, s)
    assert rz["gate"] == 2 and np.isnan(rz["average_parallax"])
    nan = c["bl"].copy()
    nan[5] = 0.0  # 0 / 0
    assert rp.solve_pair(nan, c["br"], s)["gate"] == 2
    # (z == 0 in ONE frame only is x / 0 = inf against a finite number: the term, the sum and the average are +inf, and
    # inf * 160 > 30 is true — the pair runs, in the reference too)
    one = rp.solve_pair(zl, c["br"], s)
    assert one["average_parallax"] == np.inf and one["gate"] in (0, 3)


def no_model_pair():
    """Two unrelated clouds of 40 bearings on which no hypothesis scores, or the winner keeps fewer than 8 inliers (gate 3)."""
    for seed in range(400):
        rng = np.random.default_rng([seed, 77])
        bl, br = gen.annulus(rng, 40, (40.0, 120.0)), gen.annulus(rng, 40, (40.0, 120.0))
        s = gen.make_samples(seed, 40, 1 + seed % 3)
        if rp.solve_pair(bl, br, s)["gate"] == 3:
            return dict(bl=bl, br=br), s
    raise AssertionError("no such pair")


def test_l_skips_gated_and_failed_pairs():
    good = gen.make_case(21, 50, noise_px=0.1, baseline=0.4)
    small = gen.make_case(22, 10)
    nm, nm_s = no_model_pair()
    still = dict(bl=good["bl"], br=good["bl"])
    S = 3
    sm = np.zeros((5, S, 8), np.int32)
    sm[1] = gen.make_samples(23, 50, S)
    sm[2, :len(nm_s)] = nm_s
    sm[2, len(nm_s):] = nm_s[0]
    sm[3] = gen.make_samples(24, 50, S)
    sm[4] = gen.make_samples(25, 50, S)
    off, bl, br = csr([small, still, nm, good, good])
    r = rp.relative_pose(off, bl, br, sm)
    assert [p["gate"] for p in r["pair"]] == [1, 2, 3, 0, 0] and r["l"] == 3
    assert np.array_equal(r["relative_R"], r["pair"][3]["rotation"]) and np.array_equal(r["relative_T"], r["pair"][3]["translation"])
    off2, bl2, br2 = csr([small, still, nm])
    assert rp.relative_pose(off2, bl2, br2, sm[:3])["l"] == -1


# ---------------------------------------------------------------------------------------------------------------- host, no device
from test_sfm_construct_host import attempt, host, stream  # noqa: E402,F401  (the fixtures and the driver of the construct tests)


def corresponding(gather, i, newest=W):
    """getCorresponding(i, newest) (feature_manager.cpp:118-137) on sfm_f as test_sfm_construct_host.sfm_f_of gathers it."""
    ids, off, frm, us = gather
    bl, br = [], []
    for j in range(len(ids)):
        start, n = int(frm[off[j]]), int(off[j + 1] - off[j])
        if start <= i and start + n - 1 >= newest:
            bl.append(us[off[j] + i - start]), br.append(us[off[j] + newest - start])
    return np.array(bl).reshape(-1, 3), np.array(br).reshape(-1, 3)


def regather(gather):
    pairs = [corresponding(gather, i) for i in range(W)]
    off = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int32)
    return off, np.vstack([p[0] for p in pairs]), np.vstack([p[1] for p in pairs])


def test_host_without_a_device(host, stream):
    """Flag on: the first full-window image gathers the ten pairs (equal to the re-gather), reports LFVIO_ERR_DEVICE before any call
    and the window slides, still initializing.  Flag off: relativePose() is never entered."""
    import torch

    if torch.cuda.is_available():
        return
    p, s, rd = stream
    k0 = host.relative_counts()
    host.set_self_relative_pose(True)
    try:
        a = attempt(host, s, rd, 10.0, lambda kf: None, first=W)
    finally:
        host.set_self_relative_pose(False)
    lr, f = host.last_relative(), host.flow()
    assert a["rc"] == -2 and a["n"] == W and lr["rc"] == -2 and not lr["called"] and lr["out"] is None and host.relative_counts() == k0
    off, bl, br = regather(a["gather"])
    assert np.array_equal(lr["offset"], off) and lr["bl"].tobytes() == bl.tobytes() and lr["br"].tobytes() == br.tobytes() and off[-1] > 20
    assert f["solver_flag"] == 0 and f["frame_count"] == W
    assert f["sum_of_back"] + f["sum_of_front"] == a["flow"]["sum_of_back"] + a["flow"]["sum_of_front"] + 1
    assert f["marginalization_flag"] == (abi.MARGIN_OLD if a["parallax_old"] else abi.MARGIN_SECOND_NEW)
    assert host.construct_counts() == a["k0"]
    # flag off: the same images slide without an attempt
    from test_pnp_host import fill_window

    _, rc = fill_window(host, s, rd, W + 3)
    assert rc == 0 and host.relative_counts() == k0 and host.last_relative()["rc"] == -2
