"""50-digit statement of the step half of one trust-region pass (test infrastructure: mpmath and numpy), the reference that
tests/test_step_hp.py holds k_backsub, k_backsub_wt, k_dogleg, k_cost, k_cost_imu, k_decide, k_step and k_stepw to, stage by stage.

Written from Ceres 1.12's formulas and the reference's — not from the kernels:

  a  back-substitution   the landmark rows of the scaled system (schur_eliminator_impl.h BackSubstitute, one 1 x 1 block per landmark):
                         e_l y_l = s_l b_l - s_l w_l . (S_c y_c),  e_l = s_l^2 a_l + mu d_l^2;  gauss_newton_l = -diagonal_l y_l
                         (dogleg_strategy.cc ComputeGaussNewtonStep); w_l . G_c and w_l . N_c, which every interpolant's model needs;
                         |gauss_newton_step_|^2 and gradient_ . gauss_newton_step_ over pose side and landmarks
  b  dogleg              dogleg_strategy.cc ComputeTraditionalDoglegStep: case 1 (Gauss-Newton step inside the radius), case 2 (the
                         Cauchy point outside it), case 3 (the interpolation, beta by the stable one of its two forms); the step is
                         cg gradient_ + cn gauss_newton_.  The `c <= 0` form of beta cannot be reached from a positive definite
                         system: with a = -alpha gradient_ (the Cauchy point) and b the Gauss-Newton step, a . (b - a) >= 0 — the model
                         decreases along the segment from a to b, and a minimizes it along -gradient_ — so c = a . (b - a) > 0 wherever
                         case 3 is entered; the device is not asked for it (dogleg_hp asserts that it was not taken)
  c  step and candidate  delta = (cg gradient_ + cn gauss_newton_) / diagonal_ * scale (trust_region_minimizer.cc: the step is undone
                         through the Jacobi scaling), zero in the constant ex / td columns; x_plus_delta by
                         pose_local_parameterization.cpp:3-19 (p + dp, (q * deltaQ(dtheta)).normalized()) for the poses and ex, plain sums
                         for speed / bias, td and the inverse depths; |x - x_plus_delta|^2, |x_plus_delta|^2; gradient_max_norm =
                         max |x - Plus(x, -g)| (EvaluateGradientAndJacobian)
  d  candidate cost      every factor at the candidate: lin_hp.visual with CauchyLoss(1.0) (rho / 2), lin_hp.imu (|r|^2 / 2, 0 for a
                         skipped factor), the prior r0 + J0 dx (lin_hp.prior_dx)
  e  model cost change   -delta . g - 1/2 delta^T H delta over the FULL system [H_pp W^T; W diag(a)], g = [g_p; b]
  f  bookkeeping         trust_region_minimizer.cc: invalid step, parameter tolerance, function tolerance, relative decrease against
                         min_relative_decrease, StepAccepted (radius by the step quality, mu), StepRejected (radius halved), in plain double
                         on the sums the device itself formed; and the outcome of a complete 50-digit pass

Every stage is evaluated on the inputs that stage of the run under test READ (the dict Engine.step_io returns, or a comparator's dict of
the same shape), so an upstream deviation is not charged twice.  Every input is a double and is taken exactly.  A deviation is reported
in eps x the sum of the absolute values of the terms of what is compared; a difference x - x' enters a square with what it cancelled
from (|x| + |x'|), to first order, as the units of tests/lin_hp.py do.

The bars at the end of the file are 16 x the worst figure of two double-precision comparators (tests/np_ref.py's factors with a LAPACK
solve, and the oracle/ build: its linearization, its schur_solve, its factor evaluations) over the case list of tests/test_step_hp.py,
per metric and class — measured on the CPU, never on a device.
"""
import mpmath as mp
import numpy as np

import lin_hp as lh
import np_ref
import solve_hp as sh

DPS = 50
mp.mp.dps = DPS
KC, KP = np_ref.KC, np_ref.KP
EPS = 2.0 ** -53
OFF_EX, OFF_TD = np_ref.OFF_EX, np_ref.OFF_TD
to_mp, to_f = sh.to_mp, sh.to_f
Q = {k: i for i, k in enumerate(sh.Q_NAMES)}
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
SUMS = ("cost", "mlin", "mquad", "dn", "xn")


def _mpf(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def _rel(x, h, unit=None):
    """|x - h| in eps of `unit` (default |h|); a reference that is exactly zero asks for exactly zero."""
    d = abs(_mpf(x) - h)
    u = abs(h) if unit is None else unit
    if u == 0:
        return 0.0 if d == 0 else np.inf
    return float(d / u) / EPS


def _worst(got, hp, unit):
    w = 0.0
    for x, h, u in zip(np.asarray(got, float).reshape(-1), np.asarray(hp, dtype=object).reshape(-1), np.asarray(unit, dtype=object).reshape(-1)):
        w = max(w, _rel(x, h, u))
    return w


def device_H(io):
    """H_pp as the solve had it: the packed matrix k_sum / k_sumb left, or — behind k_linw — assembled in 50 digits from its sources."""
    if io["linw"] != 1:
        return sh.packed_lower(io["H"])
    vis = sh.packed_lower(io["H"][:KC * (KC + 1) // 2], KC)
    return sh.assemble_hp(vis, io["imu_out"][:, :900].reshape(10, 30, 30), io["prior_A"], io["prior_cmap"], io["est_ex"], io["est_td"])


# ------------------------------------------------------------------------------------------------------------------------
# a. back-substitution
# ------------------------------------------------------------------------------------------------------------------------
def backsub_report(io):
    """d1, d2, gn_l per landmark and the two totals against 50 digits on a, b, W, uc_grad, uc_gn, scale_l, einv_l, diag_l, grad_l and
    the pose-side q's the run read.  The totals are formed from the run's OWN gn_l (its deviation is charged to gn_l, once)."""
    N = len(io["a"])
    ug, un = to_mp(io["uc_grad"][:KC]), to_mp(io["uc_gn"][:KC])
    aug, aun = np.abs(io["uc_grad"][:KC]), np.abs(io["uc_gn"][:KC])
    rep = dict(d1=0.0, d2=0.0, gn_l=0.0)
    for l in range(N):
        nz = np.nonzero(io["W"][l])[0]
        w = [mp.mpf(float(io["W"][l, k])) for k in nz]
        aw = np.abs(io["W"][l, nz])
        d1, d2 = mp.fdot(w, [ug[k] for k in nz]), mp.fdot(w, [un[k] for k in nz])
        u1, u2 = float(aw @ aug[nz]), float(aw @ aun[nz])
        rep["d1"], rep["d2"] = max(rep["d1"], _rel(io["d1"][l], d1, u1)), max(rep["d2"], _rel(io["d2"][l], d2, u2))
        s, b, einv, dg = (mp.mpf(float(io[k][l])) for k in ("scale_l", "b", "einv_l", "diag_l"))
        # s_l w_l . (S_c y_c) = -s_l (w_l . N_c): N_c = -S_c y_c is the unscaled Gauss-Newton direction of the camera side
        y = (s * b + s * d2) * einv
        unit = abs(dg * einv * s) * (abs(b) + u2)
        rep["gn_l"] = max(rep["gn_l"], _rel(io["gn_l"][l], -dg * y, unit))
    gn, gr = to_mp(io["gn_l"]), to_mp(io["grad_l"])
    q = io["head"]["q"]
    gn2 = _mpf(q[Q["Q_GN_SQ"]]) + mp.fdot(list(gn), list(gn))
    ggn = _mpf(q[Q["Q_GRAD_GN"]]) + mp.fdot(list(gr), list(gn))
    rep["gn_sq_total"] = _rel(io["head"]["gn_sq_total"], gn2)
    rep["grad_gn_total"] = _rel(io["head"]["grad_gn_total"], ggn, abs(q[Q["Q_GRAD_GN"]]) + float(np.abs(io["grad_l"]) @ np.abs(io["gn_l"])))
    return rep


BACKSUB_METRICS = ("d1", "d2", "gn_l", "gn_sq_total", "grad_gn_total")


# ------------------------------------------------------------------------------------------------------------------------
# b. ComputeTraditionalDoglegStep
# ------------------------------------------------------------------------------------------------------------------------
def dogleg_hp(grad_sq, gn_sq, grad_gn, alpha, radius):
    """(case, cg, cn, |step|, margins, unit of cn) in 50 digits; margins = (|gn| / r - 1, alpha |g| / r - 1): how far the two tests are
    from equality; the unit of cn = beta in case 3 is (r^2 + |a|^2) / (d + c), what r^2 - |a|^2 cancels from (None: relative)."""
    grad_sq, gn_sq, grad_gn, alpha, radius = (_mpf(v) for v in (grad_sq, gn_sq, grad_gn, alpha, radius))
    gnorm, gnn = mp.sqrt(grad_sq), mp.sqrt(gn_sq)
    margins = (float(gnn / radius - 1), float(alpha * gnorm / radius - 1))
    if gnn <= radius:
        return 1, mp.mpf(0), mp.mpf(1), gnn, margins, None
    if gnorm * alpha >= radius:
        return 2, -(radius / gnorm), mp.mpf(0), radius, margins, None
    b_dot_a = -alpha * grad_gn
    a2 = (alpha * gnorm) ** 2
    bma2 = a2 - 2 * b_dot_a + gnn ** 2
    c = b_dot_a - a2
    assert c > 0, "the c <= 0 form of beta: not reachable from a positive definite system"
    d = mp.sqrt(c * c + bma2 * (radius ** 2 - a2))
    beta = (radius * radius - a2) / (d + c)
    cg, cn = -alpha * (1 - beta), beta
    return 3, cg, cn, mp.sqrt(cg * cg * grad_sq + 2 * cg * cn * grad_gn + cn * cn * gn_sq), margins, (radius * radius + a2) / (d + c)


def dogleg_double(grad_sq, gn_sq, grad_gn, alpha, radius):
    """The same in double, as tests/np_ref.py's solve states it (a comparator): cg, cn, |step|."""
    gnorm, gnn = np.sqrt(grad_sq), np.sqrt(gn_sq)
    if gnn <= radius:
        return 0.0, 1.0, gnn
    if gnorm * alpha >= radius:
        return -(radius / gnorm), 0.0, radius
    b_dot_a = -alpha * grad_gn
    a2 = (alpha * gnorm) ** 2
    bma2 = a2 - 2 * b_dot_a + gnn ** 2
    c = b_dot_a - a2
    d = np.sqrt(c * c + bma2 * (radius ** 2 - a2))
    beta = (d - c) / bma2 if c <= 0 else (radius * radius - a2) / (d + c)
    cg, cn = -alpha * (1 - beta), beta
    return cg, cn, np.sqrt(cg * cg * grad_sq + 2.0 * cg * cn * grad_gn + cn * cn * gn_sq)


def case_of(cg, cn):
    return 1 if (cg == 0.0 and cn == 1.0) else 2 if cn == 0.0 else 3


def dogleg_report(io):
    """cg, cn, |step| of every candidate z (radius / 2^z) against 50 digits on the totals the run formed; `cases` and `margins` per z.
    In case 3 cn = beta in eps of what its numerator cancels from and cg in eps of alpha (1 + that); otherwise, and |step|, relative."""
    h = io["head"]
    rep = dict(cg=0.0, cn=0.0, sn=0.0, cases=[], dev_cases=[], margins=[])
    for z in range(io["spec"]):
        case, cg, cn, sn, mg, ucn = dogleg_hp(h["grad_sq_total"], h["gn_sq_total"], h["grad_gn_total"], h["alpha"], np.ldexp(h["radius"], -z))
        c = io["coef"][z]
        rep["cases"].append(case), rep["dev_cases"].append(case_of(c[0], c[1])), rep["margins"].append(mg)
        rep["cg"] = max(rep["cg"], _rel(c[0], cg, abs(_mpf(h["alpha"])) * (1 + ucn) if case == 3 else None))
        rep["cn"], rep["sn"] = max(rep["cn"], _rel(c[1], cn, ucn)), max(rep["sn"], _rel(c[2], sn))
    return rep


DOGLEG_METRICS = ("cg", "cn", "sn")


# ------------------------------------------------------------------------------------------------------------------------
# c. the step in the ambient space, Plus(x, delta)
# ------------------------------------------------------------------------------------------------------------------------
def active_pose(est_ex, est_td):
    return sh.active_columns(est_ex, est_td)


def delta_hp(io, cg, cn):
    """delta [172] and delta_l [N] with their units (what cg gradient_ + cn gauss_newton_ cancels from, through the same scaling)."""
    cg, cn = _mpf(cg), _mpf(cn)
    act = active_pose(io["est_ex"], io["est_td"])
    gr, gn, dg, sc = (to_mp(io[k]) for k in ("grad_p", "gn_p", "diag_p", "scale_p"))
    d = (cg * gr + cn * gn) / dg * sc
    u = (abs(cg) * np.abs(gr) + abs(cn) * np.abs(gn)) / dg * sc
    for i in range(KP):
        if not act[i]:
            d[i] = u[i] = mp.mpf(0)
    if len(io["a"]) == 0:
        return d, u, to_mp(np.zeros(0)), to_mp(np.zeros(0))
    gr, gn, dg, sc = (to_mp(io[k]) for k in ("grad_l", "gn_l", "diag_l", "scale_l"))
    return d, u, (cg * gr + cn * gn) / dg * sc, (abs(cg) * np.abs(gr) + abs(cn) * np.abs(gn)) / dg * sc


def pose_plus_hp(x, d, ud):
    """pose_local_parameterization.cpp Plus: x [7] (p, q as x y z w), d [6]; returns x_plus_delta [7] and its unit [7]."""
    x, out, unit = to_mp(x), lh._zeros(7), lh._zeros(7)
    out[:3] = x[:3] + d[:3]
    unit[:3] = np.abs(x[:3]) + ud[:3]
    q, dq = lh._pose_q(x), lh._deltaQ(d[3:6])
    p = lh._qmul(q, dq)
    n = lh._norm(p)
    p = p / n
    out[3:7] = [p[1], p[2], p[3], p[0]]
    aq, adq = np.abs(q), np.abs(dq)
    adq = adq + lh._arr([0, ud[3] / 2, ud[4] / 2, ud[5] / 2])
    # |q| x |dq|: the four products of every entry, each with its absolute value
    ap = lh._arr([aq[0] * adq[0] + aq[1] * adq[1] + aq[2] * adq[2] + aq[3] * adq[3],
                  aq[0] * adq[1] + aq[1] * adq[0] + aq[2] * adq[3] + aq[3] * adq[2],
                  aq[0] * adq[2] + aq[2] * adq[0] + aq[3] * adq[1] + aq[1] * adq[3],
                  aq[0] * adq[3] + aq[3] * adq[0] + aq[1] * adq[2] + aq[2] * adq[1]]) / n
    unit[3:7] = [ap[1], ap[2], ap[3], ap[0]]
    return out, unit


def plus_hp(x, d, ud, est_ex, est_td):
    """Plus(x, delta) of the pose side: x a dict(pose, sb, ex, td) of doubles; returns the candidate and its units as dicts of mpf."""
    c, u = dict(pose=lh._zeros(11, 7), sb=lh._zeros(11, 9)), dict(pose=lh._zeros(11, 7), sb=lh._zeros(11, 9))
    for f in range(11):
        c["pose"][f], u["pose"][f] = pose_plus_hp(x["pose"][f], d[6 * f:6 * f + 6], ud[6 * f:6 * f + 6])
        o = np_ref.off_sb(f)
        c["sb"][f] = to_mp(x["sb"][f]) + d[o:o + 9]
        u["sb"][f] = np.abs(to_mp(x["sb"][f])) + ud[o:o + 9]
    if est_ex:
        c["ex"], u["ex"] = pose_plus_hp(x["ex"], d[OFF_EX:OFF_EX + 6], ud[OFF_EX:OFF_EX + 6])
    else:
        c["ex"], u["ex"] = to_mp(x["ex"]), lh._zeros(7)
    c["td"] = _mpf(x["td"]) + (d[OFF_TD] if est_td else 0)
    u["td"] = abs(_mpf(x["td"])) + ud[OFF_TD] if est_td else mp.mpf(0)
    return c, u


def _sq_diff(x, c):
    """sum (x - c)^2 and its unit: a square of a difference enters with what the difference cancelled from."""
    x, c = to_mp(np.asarray(x, float).reshape(-1)), to_mp(np.asarray(c, float).reshape(-1))
    d = x - c
    return mp.fsum(v * v for v in d), mp.fsum(v * v + 2 * abs(v) * (abs(a) + abs(b)) for v, a, b in zip(d, x, c))


def ambient(st, est_ex, est_td):
    """The parameter blocks Ceres keeps in the program, as one vector: poses, speed / bias, ex and td where they are estimated."""
    parts = [np.asarray(st["pose"], float).ravel(), np.asarray(st["sb"], float).ravel()]
    if est_ex:
        parts.append(np.asarray(st["ex"], float))
    if est_td:
        parts.append(np.array([st["td"]]))
    return np.concatenate(parts)


def candidate_report(io, states):
    """states: dict(x=, cand=[...]) of Engine.state_dict's dicts.  The pose-side step (candidate 0), every candidate entry by entry, the
    inverse depths, the four norms' sums and gradient_max_norm."""
    est_ex, est_td = io["est_ex"], io["est_td"]
    rep = dict(delta=0.0, cand_p=0.0, cand_q=0.0, cand_lam=0.0, step_sq_pose=0.0, xn2_pose=0.0, dn=0.0, xn=0.0, exact=True)
    x = states["x"]
    xa = ambient(x, est_ex, est_td)
    for z in range(io["spec"]):
        cg, cn = io["coef"][z][0], io["coef"][z][1]
        d, ud, dl, udl = delta_hp(io, cg, cn)
        if z == 0:
            rep["delta"] = _worst(io["step_p"], d, ud)
        c, u = plus_hp(x, d, ud, est_ex, est_td)
        got = states["cand"][z]
        rep["cand_p"] = max(rep["cand_p"], _worst(got["pose"][:, :3], c["pose"][:, :3], u["pose"][:, :3]), _worst(got["sb"], c["sb"], u["sb"]),
                            _worst(got["ex"][:3], c["ex"][:3], u["ex"][:3]), _rel(got["td"], c["td"], u["td"]))
        rep["cand_q"] = max(rep["cand_q"], _worst(got["pose"][:, 3:], c["pose"][:, 3:], u["pose"][:, 3:]), _worst(got["ex"][3:], c["ex"][3:], u["ex"][3:]))
        # constant blocks are copied, bit for bit
        rep["exact"] = rep["exact"] and (est_ex or np.array_equal(got["ex"], x["ex"])) and (est_td or got["td"] == x["td"])
        lam = to_mp(io["lam"])
        rep["cand_lam"] = max(rep["cand_lam"], _worst(io["cand_lam"][z], lam + dl, np.abs(lam) + udl)) if len(lam) else rep["cand_lam"]
        # the norms, from the candidate the run itself formed
        ca = ambient(got, est_ex, est_td)
        s2, u2 = _sq_diff(xa, ca)
        rep["step_sq_pose"] = max(rep["step_sq_pose"], _rel(io["coef"][z][3], s2, u2))
        rep["xn2_pose"] = max(rep["xn2_pose"], _rel(io["coef"][z][4], mp.fsum(_mpf(v) ** 2 for v in ca)))
        sums = io["block_sums"][z].sum(axis=0) if io["block_sums"].shape[1] else np.zeros(5)
        s2, u2 = _sq_diff(io["lam"], io["cand_lam"][z])
        rep["dn"] = max(rep["dn"], _rel(sums[3], s2, u2))
        rep["xn"] = max(rep["xn"], _rel(sums[4], mp.fsum(_mpf(v) ** 2 for v in io["cand_lam"][z])))
    # gradient_max_norm = max |x - Plus(x, -g)| over the program's blocks (the landmarks': |b_l|)
    g = to_mp(io["gp"])
    act = active_pose(est_ex, est_td)
    for i in range(KP):
        if not act[i]:
            g[i] = mp.mpf(0)
    c, _ = plus_hp(x, -g, np.abs(g), est_ex, est_td)
    diffs = [abs(_mpf(a) - b) for a, b in zip(xa, np.concatenate([np.asarray(c["pose"], object).ravel(), np.asarray(c["sb"], object).ravel()]
                                                                  + ([c["ex"]] if est_ex else []) + ([[c["td"]]] if est_td else [])))]
    gm = max(diffs + [mp.mpf(float(v)) for v in np.abs(io["b"])])
    rep["gmax"] = _rel(io["head"]["gmax_pose"], gm, gm + float(np.abs(xa).max()))
    return rep


CANDIDATE_METRICS = ("delta", "cand_p", "cand_q", "cand_lam", "step_sq_pose", "xn2_pose", "dn", "xn", "gmax")


# ------------------------------------------------------------------------------------------------------------------------
# d. the candidate's cost at every factor
# ------------------------------------------------------------------------------------------------------------------------
class CandState:
    """A candidate as lin_hp's factors take a state: pose [11, 7], sb [11, 9], ex [7], td, lam [N] in the CALLER's landmark order."""

    def __init__(self, st, lam):
        self.pose, self.sb, self.ex = to_mp(st["pose"]), to_mp(st["sb"]), to_mp(st["ex"])
        self.td, self.lam = mp.mpf(float(st["td"])), to_mp(lam)

    def block(self, kind, frame):
        return (self.pose[frame], self.sb[frame], self.ex, lh._arr([self.td]))[kind]


_sqrt_info = {}


def imu_cost_hp(w, f, st):
    """|sqrt_info r|^2 / 2 of IMU factor f at the state and its unit; sqrt_info from a 50-digit inverse and Cholesky factor, once per factor."""
    pre = w.imu[f]
    key = bytes(np.asarray(pre.covariance[:], float).tobytes())
    fld = lh.pre_fields(pre)
    if key not in _sqrt_info:
        _sqrt_info[key] = lh.sqrt_info(fld["P"])
    S = _sqrt_info[key]
    G = to_mp(np.asarray(w.g, float))
    r, _, abs_r, _ = lh.imu_raw(fld, G, st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1], want_J=False)
    r, ur = S.dot(r), to_f(np.abs(S).dot(abs_r))
    ar = np.abs(to_f(r))
    return r.dot(r) / 2, float(lh.product_unit(ar, ur, ar, ur)) / 2


def prior_cost_hp(w, st):
    pr = w.prior
    n = pr.n
    J0, r0 = pr.J(), pr.r()
    dx, _ = lh.prior_dx(pr, st)
    Jm = to_mp(J0)
    dxl = list(dx)
    r = lh._arr([mp.mpf(float(r0[i])) + mp.fdot(list(Jm[i]), dxl) for i in range(n)])
    # dx = x - x0 (and the vector part of q0^-1 q) cancels from |x| + |x0|: the unit of an entry of dx
    udx = np.zeros(n)
    for i in range(pr.num_blocks):
        kind, frame, idx = pr.blocks[i].kind, pr.blocks[i].frame, pr.block_idx[i]
        x0 = np.abs(np.array(pr.block_x0[i][:]))
        x = np.abs(to_f(st.block(kind, frame)))
        if kind in (0, 2):
            udx[idx:idx + 3] = x[:3] + x0[:3]
            udx[idx + 3:idx + 6] = 2.0 * float(np.abs(x0[3:7]).sum()) * float(np.abs(x[3:7]).max())
        else:
            sz = 9 if kind == 1 else 1
            udx[idx:idx + sz] = x[:sz] + x0[:sz]
    ur = np.abs(r0) + np.abs(J0) @ udx
    ar = np.abs(to_f(r))
    return r.dot(r) / 2, float(lh.product_unit(ar, ur, ar, ur)) / 2


def cost_hp(w, st_dict, lam_dev, perm):
    """Every factor of the window at the candidate (st_dict: Engine.state_dict's; lam_dev: inverse depths in DEVICE order, perm: device
    -> caller).  Returns per landmark (device order) the cost rho / 2 of its track and the unit, per IMU factor and for the prior the same."""
    N = w.N
    lam = np.zeros(N)
    lam[perm] = lam_dev
    st, obs = CandState(st_dict, lam), lh.obs_mp(w)
    inv = np.zeros(N, np.int64)
    inv[perm] = np.arange(N)
    vis, uvis = lh._zeros(N), np.zeros(N)
    for l, o0, o, fi, fj in lh.observations(w):
        r, _, abs_r, _ = lh.visual_of(w, st, l, o0, o, fi, fj, obs, want_J=False)
        s = r.dot(r)
        c = mp.log(1 + s) / 2
        vis[inv[l]] += c
        uvis[inv[l]] += float(c) + float(np.abs(to_f(r)) @ abs_r) / (1.0 + float(s))  # d(rho / 2) = r . dr / (1 + s)
    imu, uimu = lh._zeros(10), np.zeros(10)
    for f in range(10):
        if not w.imu[f].sum_dt > 10.0:
            imu[f], uimu[f] = imu_cost_hp(w, f, st)
    prior, uprior = mp.mpf(0), 0.0
    if w.prior is not None and w.prior.valid:
        prior, uprior = prior_cost_hp(w, st)
    return dict(vis=vis, uvis=uvis, imu=imu, uimu=uimu, prior=prior, uprior=uprior)


_cost_cache = {}


def cost_report(io, w, perm, states):
    """Per candidate: the visual cost per landmark block as the run reports it and in total, every IMU factor, the prior.  A run that
    reports the window's total in block 0 (k_stepw) is compared in total only."""
    rep = dict(vis_block=0.0, vis_total=0.0, imu_cost=0.0, prior_cost=0.0, skipped_zero=True)
    N, nb = w.N, io["block_sums"].shape[1]
    for z in range(io["spec"]):
        key = (id(w), np.asarray(io["cand_x"][z]).tobytes(), np.asarray(io["cand_lam"][z]).tobytes())
        if key not in _cost_cache:
            _cost_cache[key] = cost_hp(w, states["cand"][z], io["cand_lam"][z], perm)
        hp = _cost_cache[key]
        got = io["block_sums"][z][:, 0]
        if N:
            if not io["stepw"]:
                for b in range(nb):
                    sl = slice(64 * b, min(64 * b + 64, N))
                    rep["vis_block"] = max(rep["vis_block"], _rel(got[b], mp.fsum(hp["vis"][sl]), float(hp["uvis"][sl].sum())))
            rep["vis_total"] = max(rep["vis_total"], _rel(got.sum(), mp.fsum(hp["vis"]), float(hp["uvis"].sum())))
        for f in range(10):
            if w.imu[f].sum_dt > 10.0:
                rep["skipped_zero"] = rep["skipped_zero"] and io["pose_cost"][z][f] == 0.0
            else:
                rep["imu_cost"] = max(rep["imu_cost"], _rel(io["pose_cost"][z][f], hp["imu"][f], hp["uimu"][f]))
        if w.prior is not None and w.prior.valid:
            rep["prior_cost"] = max(rep["prior_cost"], _rel(io["pose_cost"][z][10], hp["prior"], hp["uprior"]))
        else:
            rep["skipped_zero"] = rep["skipped_zero"] and io["pose_cost"][z][10] == 0.0
    return rep


COST_METRICS = ("vis_block", "vis_total", "imu_cost", "prior_cost")


# ------------------------------------------------------------------------------------------------------------------------
# e. the model cost change
# ------------------------------------------------------------------------------------------------------------------------
def model_double(q, cg, cn, mlin, mquad):
    """What the bookkeeping forms from the pose-side forms and the landmark sums (plain double)."""
    lin = cg * q[Q["Q_gG"]] + cn * q[Q["Q_gN"]] + mlin
    quad = cg * cg * q[Q["Q_GG"]] + 2.0 * cg * cn * q[Q["Q_GN"]] + cn * cn * q[Q["Q_NN"]] + mquad
    return -lin - 0.5 * quad


def model_report(io, H=None):
    """-delta . g - 1/2 delta^T H delta over the full system at the run's own cg, cn, per candidate, against what its bookkeeping forms
    from q[], mlin, mquad; and the landmark sums mlin, mquad themselves against 50 digits on the d1, d2 the run wrote."""
    H = device_H(io) if H is None else H
    Hm = H if isinstance(np.asarray(H, dtype=object)[0, 0], mp.mpf) else to_mp(H)
    rows = [list(r) for r in Hm]
    aH = np.abs(to_f(Hm))
    N = len(io["a"])
    g, b, a, W = to_mp(io["gp"]), to_mp(io["b"]), to_mp(io["a"]), io["W"]
    rep = dict(mcc=0.0, mlin=0.0, mquad=0.0, values=[])
    for z in range(io["spec"]):
        cg, cn = io["coef"][z][0], io["coef"][z][1]
        d, _, dl, _ = delta_hp(io, cg, cn)
        df, dlf = np.abs(to_f(d)), np.abs(to_f(dl))
        Hd = sh._matvec(rows, d)
        lin = sh._dot(d, g) + (sh._dot(dl, b) if N else 0)
        quad = sh._dot(d, Hd)
        ulin = float(df @ np.abs(io["gp"])) + (float(dlf @ np.abs(io["b"])) if N else 0.0)
        uquad = float(df @ aH @ df)
        wd = lh._zeros(N)
        for l in range(N):
            nz = np.nonzero(W[l])[0]
            wd[l] = mp.fdot([mp.mpf(float(W[l, k])) for k in nz], [d[k] for k in nz])
        if N:
            quad += 2 * sh._dot(dl, wd) + mp.fsum(a[l] * dl[l] * dl[l] for l in range(N))
            uquad += 2.0 * float(dlf @ (np.abs(W) @ df[:KC])) + float(np.abs(io["a"]) @ (dlf * dlf))
        mcc = -lin - quad / 2
        sums = io["block_sums"][z].sum(axis=0) if io["block_sums"].shape[1] else np.zeros(5)
        got = model_double(io["head"]["q"], cg, cn, sums[1], sums[2])
        rep["mcc"] = max(rep["mcc"], _rel(got, mcc, ulin + uquad / 2))
        rep["values"].append((got, float(mcc)))
        if N:
            # the landmark sums from the run's own d1, d2 (w_l . delta_c = cg d1_l + cn d2_l)
            cgm, cnm = _mpf(cg), _mpf(cn)
            wdd = cgm * to_mp(io["d1"]) + cnm * to_mp(io["d2"])
            uwd = abs(cg) * np.abs(io["d1"]) + abs(cn) * np.abs(io["d2"])
            rep["mlin"] = max(rep["mlin"], _rel(sums[1], sh._dot(dl, b), float(dlf @ np.abs(io["b"]))))
            rep["mquad"] = max(rep["mquad"], _rel(sums[2], 2 * sh._dot(dl, wdd) + mp.fsum(a[l] * dl[l] * dl[l] for l in range(N)),
                                                  2.0 * float(dlf @ uwd) + float(np.abs(io["a"]) @ (dlf * dlf))))
    return rep


MODEL_METRICS = ("mcc", "mlin", "mquad")


# ------------------------------------------------------------------------------------------------------------------------
# f. the bookkeeping of trust_region_minimizer.cc, in plain double, on the sums the run formed
# ------------------------------------------------------------------------------------------------------------------------
def candidate_sums(io):
    """[spec][5]: the landmark blocks summed in double on the host (cost, mlin, mquad, dn, xn), the cost with the eleven pose-side ones."""
    out = np.zeros((io["spec"], 5))
    for z in range(io["spec"]):
        if io["block_sums"].shape[1]:
            out[z] = io["block_sums"][z].sum(axis=0)
        out[z][0] += io["pose_cost"][z].sum()
    return out


def bookkeeping_double(head, coef, sums, min_relative_decrease=1e-3, parameter_tolerance=1e-8, min_radius=1e-32):
    """TrustRegionMinimizer::Minimize's loop body behind the step, once per evaluated candidate, candidate z being the step for radius /
    2^z: a rejected step halves the radius and the next candidate is the step Ceres would compute for it; the walk ends at the first
    accepted, invalid or terminating one.  head: the header's fields as a dict; coef [K][5] = cg, cn, |step|, step_sq_pose, xn2_pose;
    sums [K][5].  Returns the header after it (dict), the pushed trace entries, the accepted candidate (-1: none) and the last one evaluated."""
    t = dict(head)
    q = head["q"]
    trace, acc_z, last_z = [], -1, 0
    for z in range(len(coef)):
        last_z = z
        cg, cn, sn, step_sq, xn2 = (float(v) for v in coef[z])
        cost_z, mlin, mquad, dn, xn = (float(v) for v in sums[z])
        it = dict(cost=t["x_cost"], cost_change=0.0, gradient_max_norm=0.0, step_norm=0.0, relative_decrease=0.0, step_is_valid=0, step_is_successful=0)
        mcc = model_double(q, cg, cn, mlin, mquad)
        t["model_cost_change"] = mcc
        finished = go_on = False
        if not mcc > 0.0:  # the step is invalid
            t["consec_invalid"] += 1
            if t["consec_invalid"] >= 5:  # max_num_consecutive_invalid_steps
                t["termination"], t["done"], finished = FAILURE, 1, True
            else:
                t["mu"] *= 10.0  # StepIsInvalid: the strategy's mu
                t["do_lin"], t["do_schur"] = 0, 1
        else:
            it["step_is_valid"] = 1
            t["consec_invalid"] = 0
            cand_cost = cost_z if np.isfinite(cost_z) else np.finfo(float).max
            t["cand_cost"] = cand_cost
            it["step_norm"] = np.sqrt(step_sq + dn)
            if it["step_norm"] <= parameter_tolerance * (t["x_norm"] + parameter_tolerance):
                t["termination"], t["done"], finished = CONVERGENCE, 1, True
            else:
                it["cost_change"] = t["x_cost"] - cand_cost
                if abs(it["cost_change"]) <= t["function_tolerance"] * t["x_cost"]:
                    t["termination"], t["done"], finished = CONVERGENCE, 1, True
                else:
                    it["relative_decrease"] = it["cost_change"] / mcc
                    if it["relative_decrease"] > min_relative_decrease:  # the step is accepted
                        t["cur"] ^= 1
                        acc_z = z
                        t["x_norm"] = np.sqrt(xn2 + xn)
                        it["step_is_successful"], it["cost"], it["gradient_max_norm"] = 1, cand_cost, np.nan
                        if it["relative_decrease"] < 0.25:  # DoglegStrategy::StepAccepted
                            t["radius"] *= 0.5
                        if it["relative_decrease"] > 0.75:
                            t["radius"] = max(t["radius"], 3.0 * sn)
                        t["mu"] = max(1e-8, 2.0 * t["mu"] / 10.0)
                        t["do_lin"], t["do_schur"], t["x_cost"] = 1, 1, cand_cost
                    else:  # StepRejected
                        t["radius"] *= 0.5
                        t["do_lin"], t["do_schur"], it["cost"] = 0, 0, cand_cost
                        go_on = True
        if finished:
            break  # Minimize() returns before the iteration is recorded
        t["num_succ" if it["step_is_successful"] else "num_unsucc"] += 1
        it["trust_region_radius"] = t["radius"]
        trace.append(it)
        t["trace_len"] += 1
        if t["iteration"] >= t["max_iter"]:
            t["termination"], t["done"] = NO_CONVERGENCE, 1
        elif t["radius"] <= min_radius:
            t["termination"], t["done"] = CONVERGENCE, 1
        t["iteration"] += 1
        if not go_on or t["done"]:
            break
    return t, trace, acc_z, last_z


INT_FIELDS = ("iteration", "cur", "do_lin", "do_schur", "done", "termination", "chol_fail", "num_succ", "num_unsucc", "consec_invalid", "trace_len", "skip_step")


def rounding_bounds(io):
    """Bounds, in absolute terms, on how far two correct double evaluations of the bookkeeping's chains can be apart (u = 2^-53; the
    device sums its blocks across a wave, the restatement one after the other; a contraction to FMA removes roundings, never adds one):
      a sum of n terms        either order is within (n - 1) u sum|terms| of the exact sum: 2 (n - 1) u sum|terms| apart
      cand_cost               n = blocks + 11 non-negative terms
      model_cost_change       lin: the sum of mlin's blocks, two products, two additions; quad: the sum of mquad's blocks, the three products
                              of three or four factors (3 u each), three additions; the halving is exact, one subtraction
      step_norm, x_norm       sqrt(pose part + a sum of blocks): the relative bound of the sum, one addition, halved by the root, + u
      cost_change             cand_cost's bound + u |cost_change|;   relative_decrease: the relative bounds of both + u
    per candidate z: dict(cand_cost, mcc, step_norm, x_norm) — absolute."""
    u = EPS
    nb = max(io["block_sums"].shape[1], 1)
    q = io["head"]["q"]
    out = []
    for z in range(io["spec"]):
        bs = io["block_sums"][z] if io["block_sums"].shape[1] else np.zeros((1, 5))
        cg, cn, sn, ssq, xn2 = io["coef"][z]
        n = nb + 11
        cost_terms = np.abs(bs[:, 0]).sum() + np.abs(io["pose_cost"][z]).sum()
        lin_terms = abs(cg * q[Q["Q_gG"]]) + abs(cn * q[Q["Q_gN"]]) + np.abs(bs[:, 1]).sum()
        quad_terms = abs(cg * cg * q[Q["Q_GG"]]) + abs(2.0 * cg * cn * q[Q["Q_GN"]]) + abs(cn * cn * q[Q["Q_NN"]]) + np.abs(bs[:, 2]).sum()
        mcc = u * ((2 * (nb - 1) + 4) * lin_terms + 0.5 * (2 * (nb - 1) + 3 * 3 + 3) * quad_terms + (lin_terms + 0.5 * quad_terms))
        sn2, xnn = ssq + bs[:, 3].sum(), xn2 + bs[:, 4].sum()
        out.append(dict(cand_cost=2 * (n - 1) * u * cost_terms, mcc=mcc, step_norm=((2 * (nb - 1) + 1) / 2 + 1) * u * np.sqrt(sn2),
                        x_norm=((2 * (nb - 1) + 1) / 2 + 1) * u * np.sqrt(xnn)))
    return out


def bookkeeping_check(io):
    """The run's header and trace after its bookkeeping against the restatement on its own sums.  Returns the list of what differs:
    integer fields, radius and mu must be equal (halving, 3 |step| from the run's own |step|, 2 mu / 10: single roundings of the same
    operands); the other doubles within rounding_bounds."""
    head, after = io["head"], io["after"]
    want, trace, acc_z, last_z = bookkeeping_double(head, io["coef"], candidate_sums(io))
    rb = rounding_bounds(io)
    b = rb[last_z]  # (cand_cost, model_cost_change, x_norm of the header belong to the last candidate evaluated)
    bad = []
    for k in INT_FIELDS:
        if after[k] != want[k]:
            bad.append((k, after[k], want[k]))
    for k in ("radius", "mu"):
        if after[k] != want[k]:
            bad.append((k, after[k], want[k]))
    tol = dict(cand_cost=b["cand_cost"], x_cost=b["cand_cost"], model_cost_change=b["mcc"], x_norm=b["x_norm"])
    for k, tl in tol.items():
        if not abs(after[k] - want[k]) <= tl:
            bad.append((k, after[k], want[k], tl))
    if len(io["trace"]) != len(trace):
        bad.append(("trace entries", len(io["trace"]), len(trace)))
    else:
        for z, (got, w) in enumerate(zip(io["trace"], trace)):
            bz = rb[z]
            cc = bz["cand_cost"] + EPS * abs(w["cost_change"])
            mcc = model_double(head["q"], io["coef"][z][0], io["coef"][z][1], *candidate_sums(io)[z][1:3])
            rd = abs(w["relative_decrease"]) * (cc / abs(w["cost_change"]) + bz["mcc"] / abs(mcc) + EPS) if w["cost_change"] != 0 else 0.0
            for k, tl in (("cost", bz["cand_cost"]), ("cost_change", cc), ("step_norm", bz["step_norm"]), ("relative_decrease", rd)):
                if not abs(got[k] - w[k]) <= tl:
                    bad.append((f"trace[{z}].{k}", got[k], w[k], tl))
            for k in ("step_is_valid", "step_is_successful", "trust_region_radius"):
                if got[k] != w[k]:
                    bad.append((f"trace[{z}].{k}", got[k], w[k]))
            if np.isnan(got["gradient_max_norm"]) != np.isnan(w["gradient_max_norm"]) or (not np.isnan(w["gradient_max_norm"]) and got["gradient_max_norm"] != 0.0):
                bad.append((f"trace[{z}].gradient_max_norm", got["gradient_max_norm"], w["gradient_max_norm"]))
    return bad, want, trace, acc_z


def outcome_of(t, trace, acc_z, radius0):
    """The discrete outcome of a pass: what was accepted, how the radius moved, how the loop ended."""
    if t["done"] and not (len(trace) and trace[-1]["step_is_successful"]) and t["termination"] == CONVERGENCE and t["radius"] > 1e-32:
        kind = "converged"
    elif acc_z >= 0:
        kind = "accepted_grown" if t["radius"] > np.ldexp(radius0, -acc_z) else "accepted_kept_or_halved"
    else:
        kind = "rejected" if len(trace) and trace[-1]["step_is_valid"] else "invalid"
    return dict(kind=kind, acc_z=acc_z, entries=len(trace), done=int(t["done"]), termination=int(t["termination"]), cur=int(t["cur"]))


# ------------------------------------------------------------------------------------------------------------------------
# the complete 50-digit pass (the outcome the device's must equal)
# ------------------------------------------------------------------------------------------------------------------------
def reference_pass(w, stm, mu, radius, K, function_tolerance=1e-6):
    """One pass at the window's state in 50 digits: the linearization of lin_hp.Statement (rounded to doubles once: 1e-16 of every entry,
    which the margins below are asserted to dwarf), the Gauss-Newton step of solve_hp, then b - e at the reference's OWN candidates and
    the bookkeeping on exact sums.  Returns outcome_of's dict plus `margins`: the relative distance of relative_decrease from 1e-3, 0.25
    and 0.75, of the two tolerance tests from equality and of 3 |step| from the radius where it decides between kept and grown, the smallest over the candidates walked; `dogleg`: (case, margins) per z."""
    import lin_cases as lc

    N = w.N
    perm = lc.device_order(w)
    lin = {k: stm.hi[k] for k in ("H", "g", "a", "b", "W")}
    sch = sh.schur_hp(lin["a"], lin["b"], lin["W"], mu)
    ref = sh.Reference(lin["H"], lin["g"], sch["C"], sch["z1"], mu, stm.active, sch)
    m, red = ref.model, ref.red
    io = dict(est_ex=int(stm.active[OFF_EX]), est_td=int(stm.active[OFF_TD]), a=lin["a"][perm], b=lin["b"][perm], W=lin["W"][perm],
              grad_p=red["grad"], gn_p=m["gn"], diag_p=red["diag"], scale_p=red["scale"])
    # landmarks, in 50 digits
    al, bl = to_mp(io["a"]), to_mp(io["b"])
    s = np.array([1 / (1 + mp.sqrt(v)) for v in al], dtype=object)
    d2 = np.array([sh._clip(si * si * ai) for si, ai in zip(s, al)], dtype=object)
    dg = np.array([mp.sqrt(v) for v in d2], dtype=object)
    mu_ = mp.mpf(float(mu))
    Nc = m["N"][:KC]
    y = lh._zeros(N)
    for l in range(N):
        nz = np.nonzero(io["W"][l])[0]
        wn = mp.fdot([mp.mpf(float(io["W"][l, k])) for k in nz], [Nc[k] for k in nz])
        y[l] = (s[l] * bl[l] + s[l] * wn) / (s[l] * s[l] * al[l] + mu_ * d2[l])
    io.update(grad_l=s * bl / dg if N else to_mp(np.zeros(0)), gn_l=-(dg * y), diag_l=dg, scale_l=s)
    gn_sq = m["Q_GN_SQ"] + sh._dot(io["gn_l"], io["gn_l"])
    ggn = m["Q_GRAD_GN"] + sh._dot(io["grad_l"], io["gn_l"])
    x = dict(pose=w.pose, sb=w.speed_bias, ex=w.ex_pose, td=float(w.td))
    xa = ambient(x, io["est_ex"], io["est_td"])
    x_norm = mp.sqrt(mp.fsum(_mpf(v) ** 2 for v in xa) + mp.fsum(_mpf(v) ** 2 for v in w.inv_depth))
    x_cost = _mpf(stm.hi["cost"]) + _mpf(stm.lo["cost"])
    Hm, gm = ref.H, to_mp(lin["g"])
    rows = [list(r) for r in Hm]
    lam = to_mp(w.inv_depth[perm]) if N else to_mp(np.zeros(0))
    t = dict(radius=_mpf(radius), done=0, termination=NO_CONVERGENCE, cur=0)
    entries, acc_z, dog, margins = [], -1, [], []
    for z in range(K):
        case, cg, cn, sn, mg, _ = dogleg_hp(m["grad_sq_total"], gn_sq, ggn, m["alpha"], np.ldexp(radius, -z))
        dog.append((case, mg))
        d = (cg * io["grad_p"] + cn * io["gn_p"]) / io["diag_p"] * io["scale_p"]
        for i in range(KP):
            if not stm.active[i]:
                d[i] = mp.mpf(0)
        dl = (cg * io["grad_l"] + cn * io["gn_l"]) / io["diag_l"] * io["scale_l"] if N else to_mp(np.zeros(0))
        c, _ = plus_hp(x, d, np.abs(d), io["est_ex"], io["est_td"])
        lc_ = lam + dl
        # the cost at the candidate, its own digits kept
        st = CandState(dict(pose=np.zeros((11, 7)), sb=np.zeros((11, 9)), ex=np.zeros(7), td=0.0), np.zeros(N))
        st.pose, st.sb, st.ex, st.td = c["pose"], c["sb"], c["ex"], c["td"]
        st.lam = lh._zeros(N)
        for i in range(N):
            st.lam[perm[i]] = lc_[i]
        cost = mp.mpf(0)
        obs = lh.obs_mp(w)
        for l, o0, o, fi, fj in lh.observations(w):
            r = lh.visual_of(w, st, l, o0, o, fi, fj, obs, want_J=False)[0]
            cost += mp.log(1 + r.dot(r)) / 2
        for f in range(10):
            if not w.imu[f].sum_dt > 10.0:
                cost += imu_cost_hp(w, f, st)[0]
        if w.prior is not None and w.prior.valid:
            cost += prior_cost_hp(w, st)[0]
        # the model
        lin_ = sh._dot(d, gm) + (sh._dot(dl, bl) if N else 0)
        quad = sh._dot(d, sh._matvec(rows, d))
        for l in range(N):
            nz = np.nonzero(io["W"][l])[0]
            quad += 2 * dl[l] * mp.fdot([mp.mpf(float(io["W"][l, k])) for k in nz], [d[k] for k in nz]) + al[l] * dl[l] * dl[l]
        mcc = -lin_ - quad / 2
        if not mcc > 0:
            entries.append(dict(valid=0, successful=0))
            break
        ca = np.concatenate([np.asarray(c["pose"], object).ravel(), np.asarray(c["sb"], object).ravel()] + ([c["ex"]] if io["est_ex"] else [])
                            + ([[c["td"]]] if io["est_td"] else []))
        step_norm = mp.sqrt(mp.fsum((_mpf(a_) - b_) ** 2 for a_, b_ in zip(xa, ca)) + mp.fsum(v * v for v in dl))
        ptol = mp.mpf(1e-8) * (x_norm + mp.mpf(1e-8))
        margins.append(float(abs(step_norm / ptol - 1)))
        if step_norm <= ptol:
            t["done"], t["termination"] = 1, CONVERGENCE
            break
        cc = x_cost - cost
        ftol = _mpf(function_tolerance) * x_cost
        margins.append(float(abs(abs(cc) / ftol - 1)) if ftol > 0 else np.inf)
        if abs(cc) <= ftol:
            t["done"], t["termination"] = 1, CONVERGENCE
            break
        rd = cc / mcc
        margins += [float(abs(rd / th - 1)) for th in (1e-3, 0.25, 0.75)]
        if rd > mp.mpf(1e-3):
            acc_z = z
            t["cur"] = 1
            r0 = t["radius"]
            if rd < 0.25:
                t["radius"] = t["radius"] / 2
            if rd > 0.75:
                margins.append(float(abs(3 * sn / t["radius"] - 1)))  # (radius kept or grown: max(radius, 3 |step|))
                t["radius"] = max(t["radius"], 3 * sn)
            entries.append(dict(valid=1, successful=1, grown=bool(t["radius"] > r0)))
            break
        t["radius"] = t["radius"] / 2
        entries.append(dict(valid=1, successful=0))
    if t["done"]:
        kind = "converged"
    elif acc_z >= 0:
        kind = "accepted_grown" if entries[-1]["grown"] else "accepted_kept_or_halved"
    else:
        kind = "rejected" if entries and entries[-1]["valid"] else "invalid"
    return dict(kind=kind, acc_z=acc_z, entries=len(entries), done=t["done"], termination=t["termination"], cur=t["cur"],
                margins=min(margins) if margins else np.inf, dogleg=dog,
                norms=dict(gn=float(mp.sqrt(gn_sq)), cauchy=float(m["alpha"] * mp.sqrt(m["grad_sq_total"]))))


# ------------------------------------------------------------------------------------------------------------------------
# the double-precision comparators: a whole pass in the shape of Engine.step_io's dict
# ------------------------------------------------------------------------------------------------------------------------
def _np_factor_costs(w, st):
    N = w.N
    vis = np.zeros(N)
    for l in range(N):
        o0, o1, fi = int(w.obs_offset[l]), int(w.obs_offset[l + 1]), int(w.start_frame[l])
        for o in range(o0 + 1, o1):
            r = np_ref.visual(bool(w.estimate_td), w.tr, w.row, w.sqrt_info, w.obs_point[o0], w.obs_point[o], w.obs_velocity[o0], w.obs_velocity[o],
                              w.obs_cur_td[o0], w.obs_cur_td[o], w.obs_uv_y[o0], w.obs_uv_y[o], st.pose[fi], st.pose[fi + o - o0], st.ex, st.lam[l], st.td)[0]
            vis[l] += 0.5 * np.log(1 + r @ r)
    imu = np.zeros(10)
    for f in range(10):
        if not w.imu[f].sum_dt > 10.0:
            r = np_ref.imu(w.imu[f], w.g, st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1])[0]
            imu[f] = 0.5 * r @ r
    prior = 0.0
    if w.prior is not None and w.prior.valid:
        r, _ = np_ref.prior_eval(w.prior, st)
        prior = 0.5 * r @ r
    return vis, imu, prior


def _oracle_factor_costs(oracle, w, st):
    N = w.N
    vis = np.zeros(N)
    for l in range(N):
        o0, o1, fi = int(w.obs_offset[l]), int(w.obs_offset[l + 1]), int(w.start_frame[l])
        for o in range(o0 + 1, o1):
            r = oracle.visual_evaluate(int(w.estimate_td), w.tr, w.row, w.sqrt_info, w.obs_point[o0], w.obs_point[o], w.obs_velocity[o0], w.obs_velocity[o],
                                       w.obs_cur_td[o0], w.obs_cur_td[o], w.obs_uv_y[o0], w.obs_uv_y[o], st.pose[fi], st.pose[fi + o - o0], st.ex,
                                       float(st.lam[l]), float(st.td))[0]
            vis[l] += 0.5 * np.log(1 + r @ r)
    imu = np.zeros(10)
    for f in range(10):
        if not w.imu[f].sum_dt > 10.0:
            r = oracle.imu_evaluate(w.imu[f], w.g, st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1])[0]
            imu[f] = 0.5 * r @ r
    prior = 0.0
    if w.prior is not None and w.prior.valid:  # (the oracle exposes no prior evaluation of its own: np_ref's)
        r, _ = np_ref.prior_eval(w.prior, st)
        prior = 0.5 * r @ r
    return vis, imu, prior


def state_of(st):
    return dict(pose=np.array(st.pose, float), sb=np.array(st.sb, float), ex=np.array(st.ex, float), td=float(st.td))


def comparator_pass(w, mu, radius, spec, oracle=None, function_tolerance=1e-6):
    """A whole pass in double, stage by stage, as the dict Engine.step_io returns (landmarks in device order) plus `states`.
    oracle None: tests/np_ref.py — its dense J^T J, a LAPACK Cholesky of the reduced system, its factors at the candidates;
    otherwise the oracle/ build — its linearization, the pose-side AND landmark y of its schur_solve, its factor evaluations."""
    import lin_cases as lc

    N = w.N
    perm = lc.device_order(w)
    lin = np_ref.linearize(w) if oracle is None else oracle.linearize(w)
    act = sh.active_columns(w.estimate_extrinsic, w.estimate_td)
    a, b, W = lin["a"][perm], lin["b"][perm], lin["W"][perm].reshape(N, KC)
    sch = sh.schur_double(a, b, W, mu)
    rd = sh.reduced_double(lin["H"], lin["g"], sch["C"], sch["z1"], mu, act)
    yo = None
    if oracle is None:
        y = sh.lapack_solve(rd["S"], rd["rhs"])
    else:
        yo = oracle.schur_step(w, mu)
        y = yo[:KP]
    md = sh.model_double(lin["H"], lin["g"], rd, y, sch)
    q = np.zeros(16)
    for k, i in Q.items():
        q[i] = md[k]
    uc_grad, uc_gn = np.zeros(80), np.zeros(80)
    uc_grad[:KC], uc_gn[:KC] = md["G"][:KC], md["N"][:KC]
    s = 1.0 / (1.0 + np.sqrt(a))
    d2 = np.clip(s * s * a, sh.MIN_DIAG, sh.MAX_DIAG)
    dg = np.sqrt(d2)
    einv = 1.0 / (s * s * a + mu * d2)
    grad_l = s * b / dg
    d1, d2v = W @ md["G"][:KC], W @ md["N"][:KC]
    yl = (s * b + s * d2v) * einv if oracle is None else yo[KP:][perm]
    gn_l = -dg * yl
    st0 = np_ref.St(w)
    x_norm = float(np.linalg.norm(st0.vec(w)))
    head = dict(radius=float(radius), mu=float(mu), x_cost=float(lin["cost"]), x_norm=x_norm, cand_cost=0.0, model_cost_change=0.0, alpha=float(md["alpha"]),
                grad_sq_total=float(md["grad_sq_total"]), gn_sq_total=float(q[Q["Q_GN_SQ"]] + gn_l @ gn_l), grad_gn_total=float(q[Q["Q_GRAD_GN"]] + grad_l @ gn_l),
                function_tolerance=function_tolerance, q=q, iteration=0, cur=0, do_lin=1, do_schur=1, done=0, termination=NO_CONVERGENCE, chol_fail=0,
                num_succ=0, num_unsucc=0, consec_invalid=0, trace_len=0, skip_step=0, spec_n=spec, max_iter=int(w.max_num_iterations))
    io = dict(est_ex=int(w.estimate_extrinsic), est_td=int(w.estimate_td), a=a, b=b, W=W, H=lin["H"], gp=lin["g"], linw=0, stepw=0, spec=spec,
              scale_p=rd["scale"], diag_p=rd["diag"], grad_p=rd["grad"], gn_p=md["gn"], uc_grad=uc_grad, uc_gn=uc_gn, q=q, scale_l=s, diag_l=dg,
              grad_l=grad_l, einv_l=einv, gn_l=gn_l, d1=d1, d2=d2v, lam=w.inv_depth[perm].copy(), head=head, lm_sum=np.zeros(16))
    nb = (N + 63) // 64
    io.update(coef=np.zeros((spec, 5)), cand_lam=np.zeros((spec, N)), block_sums=np.zeros((spec, nb, 5)), pose_cost=np.zeros((spec, 11)),
              cand_x=np.zeros((spec, 184)))
    states = dict(x=state_of(st0), cand=[])
    xa = st0.vec(w)[:len(st0.vec(w)) - N]
    gm = np.where(act, lin["g"], 0.0)
    xp = np_ref.plus(w, st0, np.concatenate([-gm, np.zeros(N)]))
    head["gmax_pose"] = float(max(np.abs(xa - xp.vec(w)[:len(xa)]).max(), np.abs(b).max() if N else 0.0))
    for z in range(spec):
        cg, cn, sn = dogleg_double(head["grad_sq_total"], head["gn_sq_total"], head["grad_gn_total"], head["alpha"], np.ldexp(radius, -z))
        dp = np.where(act, (cg * rd["grad"] + cn * md["gn"]) / rd["diag"] * rd["scale"], 0.0)
        dl = (cg * grad_l + cn * gn_l) / dg * s
        if z == 0:
            io["step_p"] = dp
        dfull = np.zeros(KP + N)
        dfull[:KP] = dp
        dfull[KP + perm] = dl
        cand = np_ref.plus(w, st0, dfull)
        ca = cand.vec(w)[:len(xa)]
        io["coef"][z] = [cg, cn, sn, float((xa - ca) @ (xa - ca)), float(ca @ ca)]
        io["cand_lam"][z] = cand.lam[perm]
        states["cand"].append(state_of(cand))
        io["cand_x"][z] = np.concatenate([cand.pose.ravel(), cand.sb.ravel(), cand.ex, [cand.td]])
        vis, imu, prior = _np_factor_costs(w, cand) if oracle is None else _oracle_factor_costs(oracle, w, cand)
        vis = vis[perm]
        lamd, lcd = io["lam"], io["cand_lam"][z]
        wd = cg * d1 + cn * d2v
        for bk in range(nb):
            sl = slice(64 * bk, min(64 * bk + 64, N))
            io["block_sums"][z, bk] = [vis[sl].sum(), (dl[sl] * b[sl]).sum(), (2.0 * dl[sl] * wd[sl] + a[sl] * dl[sl] * dl[sl]).sum(),
                                       ((lamd[sl] - lcd[sl]) ** 2).sum(), (lcd[sl] ** 2).sum()]
        io["pose_cost"][z, :10], io["pose_cost"][z, 10] = imu, prior
    after, trace, acc_z, _ = bookkeeping_double(head, io["coef"], candidate_sums(io))
    io.update(after=after, trace=trace, acc_z=acc_z, states=states, head_valid=1)
    return io


def full_report(io, w, perm, states, H=None):
    rep = {}
    rep.update(backsub_report(io))
    dr = dogleg_report(io)
    rep.update(dr)
    rep.update(candidate_report(io, states))
    rep.update(cost_report(io, w, perm, states))
    rep.update(model_report(io, H))
    return rep


ALL_METRICS = BACKSUB_METRICS + DOGLEG_METRICS + CANDIDATE_METRICS + COST_METRICS + MODEL_METRICS
MARGIN = 16.0
# The metrics in eps of a sum of absolute terms that involve neither y nor mu's effect on the conditioning are pooled over the classes, as
# solve_hp.POOLED is; the rest — what carries the Gauss-Newton step — has a bar per class (group, mu).
POOLED = ("d1", "cg", "cn", "sn", "cand_q", "step_sq_pose", "xn2_pose", "dn", "xn", "gmax", "vis_block", "vis_total", "imu_cost", "prior_cost", "gn_sq_total")

# Worst figure of each metric over the two comparators per case class of tests/test_step_hp.py, as its CPU tests print them
# (test_comparator_table_reproduces asserts that this table is what they give).  A bar is MARGIN x this.  Never a device figure.
COMPARATOR_WORST = {('regular', 1e-08): {'d2': 1.65,
                      'gn_l': 2.57,
                      'grad_gn_total': 0.597,
                      'delta': 2.68,
                      'cand_p': 2.86,
                      'cand_lam': 2.18,
                      'mcc': 2.77,
                      'mlin': 2.28,
                      'mquad': 1.38},
 'all': {'d1': 3.58,
         'gn_sq_total': 0.858,
         'cg': 1.25,
         'cn': 1.48,
         'sn': 1.95,
         'cand_q': 4.78,
         'step_sq_pose': 1.9,
         'xn2_pose': 3.97,
         'dn': 0.705,
         'xn': 1.86,
         'gmax': 0.0,
         'vis_block': 1.99,
         'vis_total': 1.03,
         'imu_cost': 0.745,
         'prior_cost': 0.00708},
 ('regular', 0.01): {'d2': 1.92,
                     'gn_l': 3.28,
                     'grad_gn_total': 0.787,
                     'delta': 2.82,
                     'cand_p': 2.52,
                     'cand_lam': 1.78,
                     'mcc': 2.57,
                     'mlin': 2.28,
                     'mquad': 1.14},
 ('weak', 1e-08): {'d2': 1.38,
                   'gn_l': 2.02,
                   'grad_gn_total': 1.11,
                   'delta': 3.08,
                   'cand_p': 2.5,
                   'cand_lam': 1.48,
                   'mcc': 1.81,
                   'mlin': 1.64,
                   'mquad': 2.3},
 ('weak', 0.01): {'d2': 0.859,
                  'gn_l': 2.73,
                  'grad_gn_total': 1.89,
                  'delta': 2.53,
                  'cand_p': 2.07,
                  'cand_lam': 1.36,
                  'mcc': 1.81,
                  'mlin': 1.38,
                  'mquad': 2.3},
 ('prior', 1e-08): {'d2': 0.937,
                    'gn_l': 1.52,
                    'grad_gn_total': 0.888,
                    'delta': 2.32,
                    'cand_p': 1.55,
                    'cand_lam': 2.02,
                    'mcc': 1.08,
                    'mlin': 1.32,
                    'mquad': 1.87},
 ('prior', 0.01): {'d2': 1.38,
                   'gn_l': 4.17,
                   'grad_gn_total': 1.15,
                   'delta': 2.66,
                   'cand_p': 0.99,
                   'cand_lam': 1.7,
                   'mcc': 1.18,
                   'mlin': 1.69,
                   'mquad': 0.859},
 ('solved', 1e-08): {'d2': 1.18,
                     'gn_l': 1.28,
                     'grad_gn_total': 0.644,
                     'delta': 2.2,
                     'cand_p': 0.937,
                     'cand_lam': 0.975,
                     'mcc': 2.45,
                     'mlin': 1.17,
                     'mquad': 1.08}}


def bar(metric, cls):
    return MARGIN * COMPARATOR_WORST["all" if metric in POOLED else cls][metric]


def failed_checks(rep, metrics, cls):
    return [(k, rep[k], bar(k, cls)) for k in metrics if not rep[k] <= bar(k, cls)]
