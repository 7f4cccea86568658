"""Writes tests/golden/pnp_hp.npz: PnP cases (world points, bearings) and the results of the 50-digit side of tests/pnp_ref.py,
rounded to double.  Run from the repository root:  python tests/golden/gen_pnp_hp.py

A case: a camera pose (R, t), x_cam = R x_w + t, with |t| up to a few metres and any rotation; n points along rays of the
annulus 40 - 120 degrees off the optical axis (so bearings with z < 0 are in) at 1 - 15 m; the bearing is the unit ray, moved
by a tangent-plane Gaussian of noise_px / 160 radians.  The regimes of the fixtures (4 cases each):

  clean      exact bearings (the unit ray rounded to double)          noisy      1 px, bearings rounded to float32 (the wire format)
  zneg       0.3 px, every bearing z < 0 (91 - 120 degrees)           zpos       0.3 px, every bearing z > 0 (40 - 89 degrees)
  annulus    0.3 px, 86 - 94 degrees: bearings through z ~ 0, where the division of M by us(i, 2) is ill-conditioned
  minimal    0.1 px, n = 6, 7, 8, 10                                  large      0.3 px, float32 bearings, n = 1000, 4096, 1000, 4096
  depthspread 0.3 px, ranges 0.3 - 60 m (log-uniform)

Stored per case: pw, us, the true pose, all three candidates' R, T and err, and their spread (largest difference of a
candidate's R / T from the winner's): after 15 Gauss-Newton steps the candidates agree to far below the test's bars or differ
by far more, and which of agreeing candidates wins is decided by rounding — the tests hold R, T and the winning error, never
the index.  make_case() is also what the GPU tests draw their other inputs from.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pnp_hp.npz")
FOCAL = 160.0
REGIMES = {
    "clean": dict(noise_px=0.0),
    "noisy": dict(noise_px=1.0, f32=True),
    "zneg": dict(noise_px=0.3, polar=(91.0, 120.0)),
    "zpos": dict(noise_px=0.3, polar=(40.0, 89.0)),
    "annulus": dict(noise_px=0.3, polar=(86.0, 94.0)),
    "minimal": dict(noise_px=0.1, n=(6, 7, 8, 10)),
    "large": dict(noise_px=0.3, f32=True, n=(1000, 4096, 1000, 4096)),
    "depthspread": dict(noise_px=0.3, depth=(0.3, 60.0)),
}
CASES_PER_REGIME = 4


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
    if sigma == 0.0:
        return b
    d = rng.normal(0.0, sigma, b.shape)
    d -= np.sum(d * b, 1, keepdims=True) * b
    o = b + d
    return o / np.linalg.norm(o, axis=1, keepdims=True)


def make_case(seed, n, noise_px=0.3, polar=(40.0, 120.0), depth=(1.0, 15.0), f32=False):
    """-> dict(pw [n, 3], us [n, 3], R, t): x_cam = R x_w + t."""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(size=3), rng.uniform(0.0, np.pi))
    t = rng.normal(size=3) * rng.uniform(0.1, 3.0)
    rays = annulus(rng, n, polar)
    rng_d = np.exp(rng.uniform(np.log(depth[0]), np.log(depth[1]), (n, 1))) if depth[1] / depth[0] > 20 else rng.uniform(depth[0], depth[1], (n, 1))
    xc = rays * rng_d
    pw = (xc - t) @ R  # R^T (x_cam - t)
    us = perturb(rng, rays, noise_px / FOCAL)
    if f32:
        us = us.astype(np.float32).astype(np.float64)
    lo, hi = np.cos(np.deg2rad(polar[1])), np.cos(np.deg2rad(polar[0]))
    if polar[0] > 90.0:
        assert np.all(us[:, 2] < 0)
    if polar[1] < 90.0:
        assert np.all(us[:, 2] > 0)
    assert lo < hi and np.all(us[:, 2] != 0)
    return dict(pw=np.ascontiguousarray(pw), us=np.ascontiguousarray(us), R=R, t=t)


def hp_case(pw, us):
    """Every recorded quantity of one case from the 50-digit restatement, rounded to double."""
    import pnp_ref as pr

    h = pr.compute_pose(pw, us, pr.HP)
    assert h["status"] == 0
    N = h["chosen"]
    spread_R = max(float(abs(x)) for c in range(3) for x in (h["R_all"][c] - h["R_all"][N]).reshape(-1))
    spread_T = max(float(abs(x)) for c in range(3) for x in (h["T_all"][c] - h["T_all"][N]).reshape(-1))
    return dict(R_all=pr.to_double(h["R_all"]), T_all=pr.to_double(h["T_all"]), err=pr.to_double(h["err"]), chosen=N,
                spread=np.array([spread_R, spread_T]))


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    out, names = {}, []
    rng = np.random.default_rng(2025)
    for regime, kw in REGIMES.items():
        for c in range(CASES_PER_REGIME):
            kwc = dict(kw)
            ns = kwc.pop("n", None)
            seed = int(rng.integers(1 << 30))
            n = int(rng.integers(30, 201)) if ns is None else ns[c]
            case = make_case(seed, n, **kwc)
            rec = hp_case(case["pw"], case["us"])
            name = f"{regime}_{c}"
            names.append(name)
            out[name + "/pw"], out[name + "/us"], out[name + "/R_true"], out[name + "/t_true"] = case["pw"], case["us"], case["R"], case["t"]
            for k, v in rec.items():
                out[name + "/" + k] = np.asarray(v)
            print(name, "n", n, "chosen", rec["chosen"], "err", rec["err"], "spread", rec["spread"],
                  "to truth", np.abs(rec["R_all"][rec["chosen"]] - case["R"]).max(), flush=True)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
