"""Restatement of Estimator::relativePose (estimator.cpp:445-473) over MotionEstimator::solveRelativeRT
(initial/solve_5pts.cpp:395-576), the reference behind tests/test_relative_pose*.py.  numpy, double precision, written from the line
references of include/lfvio.h on top of tests/twoview_ref.py: compute_E_21, check_inliers, myfindFundamentalMat, decomposeEssentialMat
and triangulatePoint of solve_5pts.cpp are the steps of initial_ex_rotation.cpp that twoview_ref.two_view restates.

  recover_pose(bl, br, R1, R2, t)            :395-535  good1..good4 over ALL matches and the >= chain
  relative_pose(offsets, bl, br, samples)    the candidate loop with its gates (:452, :464), every pair evaluated; the fields of
                                             LfvioRelativePoseOut, and per pair two_view's condition facts and `gap`

The output is the INTENDED one (include/lfvio.h, deviation 1): rotation = rot^T, translation = -rot^T trans.
"""
import numpy as np

import twoview_ref as tv

MIN_MATCHES = 20  # a pair runs when N > 20 (:452)


def choose(good):
    """:507-534: the >= chain, in that order."""
    g1, g2, g3, g4 = (int(g) for g in good)
    if g1 >= g2 and g1 >= g3 and g1 >= g4:
        return 0
    if g2 >= g1 and g2 >= g3 and g2 >= g4:
        return 1
    if g3 >= g1 and g3 >= g2 and g3 >= g4:
        return 2
    return 3


def good_count(bl, br, R, t):
    """:430-449 for one candidate: triangulatePoint's null vector divided by its fourth entry; the match counts when both dot products
    divided by the point's norms are > 0 (a non-finite point does not count)."""
    Vt = np.linalg.svd(tv.design(bl, br, R, t))[2]
    with np.errstate(all="ignore"):
        Q = Vt[:, 3, :3] / Vt[:, 3, 3:4]
        Q2 = Q @ R.T + t
        dl = np.einsum("ni,ni->n", bl, Q) / np.sqrt(np.einsum("ni,ni->n", Q, Q))
        dr = np.einsum("ni,ni->n", br, Q2) / np.sqrt(np.einsum("ni,ni->n", Q2, Q2))
        return int(np.count_nonzero((dl > 0) & (dr > 0)))


def candidates(R1, R2, t):
    """recoverPose's order: (R1, t) (R2, t) (R1, -t) (R2, -t)."""
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def recover_pose(bl, br, R1, R2, t):
    """-> (good[4], chosen)."""
    bl, br = np.asarray(bl, np.float64), np.asarray(br, np.float64)
    good = np.array([good_count(bl, br, R, tt) for R, tt in candidates(np.asarray(R1), np.asarray(R2), np.asarray(t))], np.int32)
    return good, choose(good)


def average_parallax(bl, br):
    """:454-463: one double, the terms added in match order."""
    with np.errstate(all="ignore"):
        dx = bl[:, 0] / bl[:, 2] - br[:, 0] / br[:, 2]
        dy = bl[:, 1] / bl[:, 2] - br[:, 1] / br[:, 2]
        terms = np.sqrt(dx * dx + dy * dy)
        s = np.float64(0.0)
        for v in terms:
            s = s + v
        return float(1.0 * s / len(bl))


def solve_pair(bl, br, samples):
    """One pair -> dict with the fields of LfvioRelativePosePair, two_view's condition facts (c1_gap, c2_margin, c3_gap, rank2, ...)
    and gap = largest minus second-largest good count."""
    bl, br = np.ascontiguousarray(bl, np.float64).reshape(-1, 3), np.ascontiguousarray(br, np.float64).reshape(-1, 3)
    N = len(bl)
    out = dict(gate=0, num_matches=N, best_sample=-1, num_inliers=0, average_parallax=0.0, best_score=0.0, chosen=-1, inlier_cnt=0, ok=0,
               good=np.zeros(4, np.int32))
    if N <= MIN_MATCHES:
        out["gate"] = 1
        return out
    out["average_parallax"] = average_parallax(bl, br)
    with np.errstate(all="ignore"):
        if not out["average_parallax"] * 160 > 30:
            out["gate"] = 2
            return out
    r = tv.two_view(bl, br, samples)
    out.update(best_sample=r["best_sample"], num_inliers=r["num_inliers"], best_score=r["best_score"])
    if r["status"] != 0:
        out["gate"] = 3
        return out
    for k in ("mask", "E", "R_cand", "t_cand", "c1_gap", "c2_margin", "c3_gap", "rank2", "cond_refit"):
        out[k] = r[k]
    out["status"] = 0
    R1, R2, t = r["R_cand"][0], r["R_cand"][1], r["t_cand"]
    good, chosen = recover_pose(bl, br, R1, R2, t)
    rot, trans = candidates(R1, R2, t)[chosen]
    srt = np.sort(good)
    out.update(good=good, chosen=chosen, inlier_cnt=int(good[chosen]), ok=int(good[chosen] > 12), gap=int(srt[3] - srt[2]),
               rot=rot.copy(), trans=trans.copy(), rotation=rot.T.copy(), translation=-(rot.T @ trans))
    return out


def relative_pose(offsets, bl, br, samples):
    """-> dict(l, relative_R, relative_T, pair [P]).  samples [P, S, 8], local to the pair; every pair is evaluated."""
    off = np.asarray(offsets, np.int64).reshape(-1)
    bl, br = np.asarray(bl, np.float64).reshape(-1, 3), np.asarray(br, np.float64).reshape(-1, 3)
    P = len(off) - 1
    samples = np.asarray(samples, np.int32).reshape(P, -1, 8)
    pair = [solve_pair(bl[off[p]:off[p + 1]], br[off[p]:off[p + 1]], samples[p]) for p in range(P)]
    l = next((p for p in range(P) if pair[p]["gate"] == 0 and pair[p]["ok"]), -1)
    return dict(l=l, relative_R=pair[l]["rotation"] if l >= 0 else None, relative_T=pair[l]["translation"] if l >= 0 else None, pair=pair)


def match_candidates(got, ref):
    """The device and the restatement may name the four candidates differently (which rotation is R1 and the sign of t follow an
    SVD's signs).  -> perm with got's candidate perm[j] being ref's candidate j, in recoverPose's order."""
    gR, rR = np.asarray(got["R_cand"]).reshape(2, 3, 3), np.asarray(ref["R_cand"]).reshape(2, 3, 3)
    swap = tv.rot_angle(gR[0], rR[0]) + tv.rot_angle(gR[1], rR[1]) > tv.rot_angle(gR[0], rR[1]) + tv.rot_angle(gR[1], rR[0])
    flip = float(np.asarray(got["t_cand"]) @ np.asarray(ref["t_cand"])) < 0
    return [(r ^ int(swap)) + 2 * (s ^ int(flip)) for s in (0, 1) for r in (0, 1)]


def direction_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), float(a @ b)))
