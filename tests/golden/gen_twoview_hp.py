"""Writes tests/golden/twoview_hp.npz: two-view cases (bearing pairs, sample sets) and the results of the 50-digit
restatement of tests/twoview_ref.py, rounded to double.  Run from the repository root:  python tests/golden/gen_twoview_hp.py

Cases: two views of random points 2 - 12 m away in the annulus 40 - 120 degrees off the optical axis (so rays with z < 0 are
in), a rotation of 0.5 - 10 degrees and a baseline between the frames; bearing noise in pixels at f = 160; gross outliers
replace the newer frame's bearing by a random one of the annulus.  The regimes of the fixtures:

  clean      0.1 px, no outliers            noisy      1 px
  outliers   0.3 px, 30 % outliers          smallbase  0.3 px, baseline 0.02 m
  zneg       0.3 px, rays with z <= 0 only  zpos       0.3 px, rays with z >= 0 only
  minimal    0.1 px, N = 8, 9, 10, 12: the refit is an (almost) square system, the worst conditioned the call meets;
             the bars of the GPU tests' smallest sizes come from here

make_case() and make_samples() are also what the GPU tests draw their other inputs from (sizes, ties, pure rotation).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "twoview_hp.npz")
REGIMES = {
    "clean": dict(noise_px=0.1, outliers=0.0),
    "noisy": dict(noise_px=1.0, outliers=0.0),
    "outliers": dict(noise_px=0.3, outliers=0.3),
    "smallbase": dict(noise_px=0.3, outliers=0.0, baseline=0.02),
    "zneg": dict(noise_px=0.3, outliers=0.1, polar=(91.0, 120.0)),
    "zpos": dict(noise_px=0.3, outliers=0.1, polar=(40.0, 89.0)),
    "minimal": dict(noise_px=0.1, outliers=0.0, N=(8, 9, 10, 12), S=6),
}
CASES_PER_REGIME = 4
SAMPLES = 24
FOCAL = 160.0


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def annulus(rng, n, polar):
    th = np.deg2rad(rng.uniform(polar[0], polar[1], n))
    ph = rng.uniform(0, 2 * np.pi, n)
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)


def perturb(rng, b, sigma):
    """Unit vectors moved by a tangent-plane Gaussian of sigma radians."""
    if sigma == 0.0:
        return b
    n = rng.normal(0.0, sigma, b.shape)
    n -= np.sum(n * b, 1, keepdims=True) * b
    o = b + n
    return o / np.linalg.norm(o, axis=1, keepdims=True)


def make_case(seed, N, noise_px=0.3, outliers=0.0, rot_deg=None, baseline=None, polar=(40.0, 120.0)):
    """-> dict(bl, br, R, t): X_r = R X_l + t, so the relative rotation solveRelativeR returns is R^T."""
    rng = np.random.default_rng(seed)
    rot_deg = rng.uniform(0.5, 10.0) if rot_deg is None else rot_deg
    baseline = rng.uniform(0.02, 0.5) if baseline is None else baseline
    R = rodrigues(rng.normal(size=3), np.deg2rad(rot_deg))
    d = rng.normal(size=3)
    t = baseline * d / np.linalg.norm(d)
    # points whose rays stay inside the annulus in both frames
    pts = np.zeros((0, 3))
    lo, hi = np.cos(np.deg2rad(polar[1])), np.cos(np.deg2rad(polar[0]))
    while len(pts) < N:
        X = annulus(rng, 2 * N, polar) * rng.uniform(2.0, 12.0, (2 * N, 1))
        Xr = X @ R.T + t
        zr = Xr[:, 2] / np.linalg.norm(Xr, axis=1)
        pts = np.vstack([pts, X[(zr >= lo) & (zr <= hi)]])
    X = pts[:N]
    Xr = X @ R.T + t
    bl = X / np.linalg.norm(X, axis=1, keepdims=True)
    br = Xr / np.linalg.norm(Xr, axis=1, keepdims=True)
    sigma = noise_px / FOCAL
    bl, br = perturb(rng, bl, sigma), perturb(rng, br, sigma)
    n_out = int(round(outliers * N))
    if n_out:
        idx = rng.choice(N, n_out, replace=False)
        br = br.copy()
        br[idx] = annulus(rng, n_out, polar)
    return dict(bl=np.ascontiguousarray(bl), br=np.ascontiguousarray(br), R=R, t=t)


def make_samples(seed, N, S, sort=False):
    """S sets of 8 distinct match indices.  sort: every set ascending, so that two draws of the same set are the same
    computation bit for bit and tie exactly (with few matches most draws repeat a set; in another order their scores
    would differ by rounding, and which of them wins would be decided by it)."""
    rng = np.random.default_rng(seed)
    s = np.stack([rng.choice(N, 8, replace=False) for _ in range(S)]).astype(np.int32)
    return np.sort(s, axis=1) if sort else s


def hp_case(bl, br, samples):
    """Every recorded quantity of one case from the 50-digit restatement."""
    import twoview_ref as tv

    S = len(samples)
    rec = dict(E_all=np.zeros((S, 9)), cond_all=np.zeros((S, 2)), score_all=np.zeros(S, np.float32))
    masks, Es = [], []
    for k, idx in enumerate(samples):
        E, cA, gap, _, _ = tv.hp_compute_E(bl[idx], br[idx])
        sc, mk, _ = tv.hp_check_inliers(E, bl, br)
        rec["E_all"][k], rec["cond_all"][k], rec["score_all"][k] = tv.hp_to_np(E).reshape(9), (float(cA), float(gap)), sc
        masks.append(mk), Es.append(E)
    best, bs = -1, 0.0
    for k in range(S):
        if bs < float(rec["score_all"][k]):
            bs, best = float(rec["score_all"][k]), k
    if best < 0 or masks[best].sum() < 8:
        return None  # no model: the generator takes the next seed (the no-model cases are a test of their own)
    _, _, m_win = tv.hp_check_inliers(Es[best], bl, br)
    sel = masks[best].astype(bool)
    E, cA, gap, rank2, _ = tv.hp_compute_E(bl[sel], br[sel])
    _, mask, m_fit = tv.hp_check_inliers(E, bl, br)
    R1, R2, t = tv.hp_decompose(E)
    fr = [tv.hp_front_count(bl, br, R1, t), tv.hp_front_count(bl, br, R1, -t), tv.hp_front_count(bl, br, R2, t), tv.hp_front_count(bl, br, R2, -t)]
    first = max(fr[0], fr[1]) > max(fr[2], fr[3])
    rec.update(best_sample=best, best_score=bs, pre_inliers=int(sel.sum()), E=tv.hp_to_np(E).reshape(9), cond_refit=np.array([float(cA), float(gap)]),
               rank2=float(rank2), mask=mask, num_inliers=int(mask.sum()), R_cand=np.stack([tv.hp_to_np(R1), tv.hp_to_np(R2)]),
               t_cand=tv.hp_to_np(t).reshape(3), front=np.array(fr, np.int32), R_rel=tv.hp_to_np(R1 if first else R2).T.copy(),
               c2_margin=min(m_win, m_fit))
    return rec


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    out, names = {}, []
    rng = np.random.default_rng(2024)
    for regime, kw in REGIMES.items():
        for c in range(CASES_PER_REGIME):
            kwc = dict(kw)
            Ns, S = kwc.pop("N", None), kwc.pop("S", SAMPLES)
            rec = None
            while rec is None:
                seed = int(rng.integers(1 << 30))
                N = int(rng.integers(30, 201)) if Ns is None else Ns[c]
                case = make_case(seed, N, **kwc)
                samples = make_samples(seed + 1, N, S, sort=Ns is not None)
                rec = hp_case(case["bl"], case["br"], samples)
            name = f"{regime}_{c}"
            names.append(name)
            out[name + "/bl"], out[name + "/br"], out[name + "/samples"] = case["bl"], case["br"], samples
            out[name + "/R_true"], out[name + "/t_true"] = case["R"], case["t"]
            for k, v in rec.items():
                out[name + "/" + k] = np.asarray(v)
            print(name, "N", N, "best", rec["best_sample"], "inliers", rec["num_inliers"], "front", rec["front"], "cond", rec["cond_all"].max(0), flush=True)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
