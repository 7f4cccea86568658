"""Writes tests/golden/sfm_ba_hp.npz: bundle-adjustment cases for lfvio_sfm_ba and the results of the 50-digit side of
tests/sfm_ba_ref.py, rounded to double.  Run from the repository root:  python tests/golden/gen_sfm_ba_hp.py  (about 10 minutes).

A scene: F cameras on a wavy line 3 m long, each turned by up to 8 degrees, and P points 4 - 9 m in front of them (`wide`:
50 - 130 degrees off the optical axis, to the sides of the line of motion, so that bearings fall on both sides of z = 0).  A bearing
is the unit ray moved by a tangent-plane Gaussian of noise_px / 160 radians.  Tracks are full, or ragged: a run of at least 3
consecutive frames per point.  The initial state is the truth with every free rotation turned by `pert[0]` degrees about a random
axis, every free translation moved by pert[1] x the length of the camera line and every point by pert[2] x its depth (Gaussian).

  f2_p6                         F = 2, P = 6, l = 0: three camera unknowns
  f3_p8_l0, f3_p8_l1            F = 3, P = 8
  f11_full                      F = 11, P = 60, full tracks, l = 3
  f11_full_wide                 bearings on both sides of z = 0
  f11_full_exact                exact bearings: a zero-residual minimum, used for the evaluation test only
  f11_full_reject               a 12 degree / 0.2 / 30 % start: rejected steps on the way
  f11_rag_l0                    ragged, and point 0 has a single observation (its depth is not determined)
  f11_rag_l4                    ragged, and frame 7 has no observation (its pose is not determined and must not move)
  f11_rag_l9                    ragged, bearings stored un-normalised (norm 1 +- 1e-3) and rounded to float32
  f11_rag_p65, f11_rag_p257     one more than a wavefront, one more than the kernel's workgroup

Stored per case: the inputs; from the 50-digit side the cost, the tangent gradient (gc [F, 6], gp [P, 3]), gradient_max_norm and the
reduced camera system (S, rhs: Jacobi-scaled, damped at radius 1e4) at the initial state, and the minimiser of the gauge-fixed
problem (the restatement's forced-convergence result polished by Gauss-Newton in 50 digits until the step is below 1e-30) as
R_min [F, 3, 3], t_min, X_min, RQ_min (the matrix of Q), T_min, cost_min; the condition number of the tangent Jacobian there (free columns; without
the columns of a frame with no observation, and without the rows and columns of a point of one observation); the margins of the
restatement's default-option trace (rho_margin_ok, dcost_margin_ok) that decide which cases the trace test may use.
The seeds are chosen so that every case with noisy bearings has both margins (margins() below; four first choices did not and were
replaced).  `python tests/golden/gen_sfm_ba_hp.py NAME ...` re-makes the named cases only and keeps the file's others.
The generator asserts: the analytic Jacobian equals a 50-digit central difference of the literal residual to 1e-30; cond <= 1e6.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sfm_ba_hp.npz")
FOCAL = 160.0
COND_CAP = 1e6
FORCE = dict(function_tolerance=1e-30, gradient_tolerance=1e-30, parameter_tolerance=1e-30)
CASES = {
    "f2_p6": dict(seed=11, F=2, P=6, l=0),
    "f3_p8_l0": dict(seed=22, F=3, P=8, l=0),
    "f3_p8_l1": dict(seed=123, F=3, P=8, l=1),
    "f11_full": dict(seed=31, F=11, P=60, l=3),
    "f11_full_wide": dict(seed=138, F=11, P=60, l=5, wide=True),
    "f11_full_exact": dict(seed=33, F=11, P=60, l=2, noise_px=0.0),
    "f11_full_reject": dict(seed=34, F=11, P=60, l=3, pert=(12.0, 0.2, 0.30)),
    "f11_rag_l0": dict(seed=142, F=11, P=60, l=0, tracks="ragged", single=True),
    "f11_rag_l4": dict(seed=42, F=11, P=60, l=4, tracks="ragged", empty_frame=7),
    "f11_rag_l9": dict(seed=146, F=11, P=60, l=9, tracks="ragged", unnormalised=True),
    "f11_rag_p65": dict(seed=44, F=11, P=65, l=6, tracks="ragged"),
    "f11_rag_p257": dict(seed=45, F=11, P=257, l=1, tracks="ragged"),
}


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quat_of(R):
    """w x y z of a rotation matrix with a positive trace + 1 (every camera here)."""
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def make_scene(seed, F, P, l, tracks="full", noise_px=1.0, wide=False, unnormalised=False, empty_frame=None, single=False, pert=(1.5, 0.03, 0.05)):
    """-> dict(F, l, off, frame, bearing, q0, t0, X0, q_true, t_true, X_true, active_c [F, 6], single [P])."""
    rng = np.random.default_rng(seed)
    k = np.arange(F)
    c = np.stack([3.0 / (F - 1) * k, 0.15 * np.sin(0.9 * k + seed), 0.1 * np.cos(0.7 * k)], 1) + rng.normal(0, 0.03, (F, 3))
    Rs = [rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0, 8))) for _ in range(F)]
    q = np.stack([quat_of(R) for R in Rs])
    t = np.stack([-R @ ci for R, ci in zip(Rs, c)])
    mid = c.mean(0)
    if wide:
        th, ph = np.deg2rad(rng.uniform(50, 130, P)), np.deg2rad(rng.uniform(45, 135, P) + 180 * rng.integers(0, 2, P))
        X = mid + rng.uniform(4, 9, (P, 1)) * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    else:
        X = mid + np.stack([rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(4, 9, P)], 1)
    off, frame = [0], []
    for i in range(P):
        if tracks == "full":
            fr = list(range(F))
        else:
            s = int(rng.integers(0, F - 3))
            n = int(rng.integers(4, F - s + 1)) if F - s >= 4 else 3
            fr = list(range(s, s + n))
        if empty_frame is not None:
            fr = [f for f in fr if f != empty_frame]
        if single and i == 0:
            fr = fr[1:2]
        frame += fr
        off.append(len(frame))
    frame = np.array(frame)
    pt = np.repeat(np.arange(P), np.diff(off))
    pc = np.einsum("mij,mj->mi", np.stack(Rs)[frame], X[pt]) + t[frame]
    b = pc / np.linalg.norm(pc, axis=1, keepdims=True)
    if noise_px > 0:
        d = rng.normal(0, noise_px / FOCAL, b.shape)
        d -= np.sum(d * b, 1, keepdims=True) * b
        b = b + d
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    if unnormalised:
        b = (b * (1 + 1e-3 * rng.normal(size=(len(b), 1)))).astype(np.float32).astype(np.float64)
    if wide:
        assert np.any(b[:, 2] < -0.1) and np.any(b[:, 2] > 0.1)
    # the start
    q0, t0, X0 = q.copy(), t.copy(), X.copy()
    line = np.linalg.norm(c[-1] - c[0])
    for f in range(F):
        if f != l:
            R0 = rodrigues(rng.normal(size=3), np.deg2rad(pert[0])) @ Rs[f]
            q0[f] = quat_of(R0)
        if f != l and f != F - 1:
            t0[f] = t[f] + pert[1] * line * rng.normal(size=3) / np.sqrt(3)
    depth = np.linalg.norm(X - mid, axis=1, keepdims=True)
    X0 = X + pert[2] * depth * rng.normal(size=(P, 3)) / np.sqrt(3)
    active = np.ones((F, 6), bool)
    if empty_frame is not None:
        active[empty_frame] = False
    return dict(F=F, l=l, off=np.array(off, np.int32), frame=frame.astype(np.int32), bearing=np.ascontiguousarray(b), q0=q0, t0=t0, X0=X0,
                q_true=q, t_true=t, X_true=X, active_c=active, single=np.diff(off) == 1)


def condition(pb, sc, q, t, X):
    """Condition number of the tangent Jacobian at (q, t, X) over what the problem determines."""
    import sfm_ba_ref as sr

    J = sr.dense_jacobian(pb, sr.evaluate(pb, q, t, X))
    n = pb["n"]
    keep_c = np.ones(J.shape[1], bool)
    keep_r = np.ones(J.shape[0], bool)
    for f in range(pb["F"]):
        for k in range(6):
            if pb["col"][f, k] >= 0 and not sc["active_c"][f, k]:
                keep_c[pb["col"][f, k]] = False
    for i in np.nonzero(sc["single"])[0]:
        keep_c[n + 3 * i:n + 3 * i + 3] = False
        for o in range(pb["off"][i], pb["off"][i + 1]):
            keep_r[3 * o:3 * o + 3] = False
    s = np.linalg.svd(J[keep_r][:, keep_c], compute_uv=False)
    return float(s[0] / s[-1])


def check_jacobian(pb, sc):
    """The analytic tangent Jacobian against a 50-digit central difference of the literal residual, on up to 12 observations."""
    import sfm_ba_ref as sr

    A, mp = sr.HP, sr.HP.mp
    q, t, X = A.arr(sc["q0"]), A.arr(sc["t0"]), A.arr(sc["X0"])
    ev = sr.evaluate(pb, q, t, X, A)
    h = mp.mpf(10) ** -20
    worst = mp.mpf(0)
    for o in list(range(min(pb["M"], 12))):
        f, i = int(pb["frame"][o]), int(pb["pt"][o])
        for k in range(9):
            def moved(sign):
                dc, dp = A.arr(np.zeros((pb["F"], 6))), A.arr(np.zeros((pb["P"], 3)))
                if k < 6:
                    dc[f, k] = sign * h
                else:
                    dp[i, k - 6] = sign * h
                return sr.evaluate(pb, *sr.plus(q, t, X, dc, dp, A), A, jac=False)["r"][o]
            num = (moved(1) - moved(-1)) / (2 * h)
            ana = ev["Jc"][o][:, k] if k < 6 else ev["Jp"][o][:, k - 6]
            worst = max(worst, max(abs(v) for v in (num - ana)))
    assert worst < mp.mpf(10) ** -30, worst
    return float(worst)


def margins(res):
    """Of a result of sfm_ba_ref.solve under default options: (every relative_decrease outside [0.5e-3, 2e-3]; every |cost_change| / cost
    that met the function-tolerance test outside [0.5e-6, 2e-6] — the valid steps of the trace, accepted or rejected, and the step that
    ended the run, which is not in the trace; where that step ended it by the parameter tolerance, its ratio outside [0.5e-8, 2e-8])."""
    trace, end = res["trace"], res["end"]
    rho_ok = all(not (0.5e-3 <= it["relative_decrease"] <= 2e-3) for it in trace[1:] if it["step_is_valid"])
    prev, dc_ok = trace[0]["cost"], True
    for it in trace[1:]:
        if it["step_is_valid"]:
            dc_ok = dc_ok and not (0.5e-6 <= abs(it["cost_change"]) / prev <= 2e-6)
        if it["step_is_successful"]:
            prev = it["cost"]
    if end is not None:
        tol = 1e-6 if end["test"] == "function" else 1e-8
        dc_ok = dc_ok and not (0.5 * tol <= end["ratio"] <= 2 * tol)
    return rho_ok, dc_ok


def hp_case(sc, log=None):
    """Every recorded quantity of one case, rounded to double."""
    import sfm_ba_ref as sr

    A = sr.HP
    pb = sr.problem(sc["F"], sc["l"], sc["off"], sc["frame"], sc["bearing"])
    rec = dict(jac_check=check_jacobian(pb, sc))
    ev = sr.evaluate(pb, sc["q0"], sc["t0"], sc["X0"], A)
    gc, gp = sr.gradient(pb, ev, A)
    s_c, s_p = sr.jacobi_scale(pb, ev, A)
    sch = sr.schur(pb, sr.blocks(pb, ev, s_c, s_p, A), A.mp.mpf(sr.INITIAL_RADIUS), A)
    rec.update(cost0=float(ev["cost"]), gc0=sr.to_double(gc), gp0=sr.to_double(gp), gmax0=float(sr.gradient_max_norm(pb, A.arr(sc["q0"]), gc, gp, A)),
               S0=sr.to_double(sch["S"]), rhs0=sr.to_double(sch["rhs"]))
    forced = sr.solve(pb, sc["q0"], sc["t0"], sc["X0"], **FORCE)
    q, t, X = sr.polish(pb, forced["c_rotation"], forced["c_translation"], forced["position"], sc["active_c"], sc["single"], log=log)
    Q, T = sr.drop_in(q, t, A)
    rec.update(R_min=sr.to_double(sr.rotation(q, A)), t_min=sr.to_double(t), X_min=sr.to_double(X), RQ_min=sr.to_double(sr.rotation(Q, A)), T_min=sr.to_double(T),
               cost_min=float(sr.evaluate(pb, q, t, X, A, jac=False)["cost"]))
    rec["cond"] = condition(pb, sc, sr.to_double(q), sr.to_double(t), sr.to_double(X))
    assert rec["cond"] <= COND_CAP, rec["cond"]
    dflt = sr.solve(pb, sc["q0"], sc["t0"], sc["X0"])
    rho_ok, dc_ok = margins(dflt)
    rec.update(rho_margin_ok=int(rho_ok), dcost_margin_ok=int(dc_ok), dflt_iterations=dflt["num_iterations"], dflt_unsuccessful=dflt["num_unsuccessful_steps"],
               forced_unsuccessful=forced["num_unsuccessful_steps"])
    return rec


def one(name):
    sys.path.insert(0, os.path.dirname(HERE))
    sc = make_scene(**CASES[name])
    rec = hp_case(sc, log=lambda s: print(name, s, flush=True))
    print(name, {k: v for k, v in rec.items() if np.ndim(v) == 0}, flush=True)
    out = {name + "/" + k: np.asarray(v) for k, v in rec.items()}
    for k in ("off", "frame", "bearing", "q0", "t0", "X0", "active_c", "single"):
        out[name + "/" + k] = np.asarray(sc[k])
    out[name + "/F"], out[name + "/l"] = np.asarray(sc["F"]), np.asarray(sc["l"])
    return out


def main():
    from multiprocessing import Pool

    names = sys.argv[1:] or list(CASES)  # with case names: only those are re-made, the file's other cases are kept as they are
    with Pool(min(len(names), 12)) as pool:
        parts = pool.map(one, names)
    out = {}
    if sys.argv[1:] and os.path.exists(OUT):
        z = np.load(OUT)
        out = {k: z[k] for k in z.files if k != "names" and k.split("/", 1)[0] not in names}
        names = [n for n in CASES if n in names or n in list(z["names"])]
    for p in parts:
        out.update(p)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
