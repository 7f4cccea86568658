"""The full BA that ends GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:233-309) restated: the reference of
tests/test_sfm_ba.py and tests/golden/gen_sfm_ba_hp.py, and what lfvio_sfm_ba (include/lfvio.h) is measured with.

One text for two arithmetics (numpy arrays of float64, or of mpmath numbers at 50 digits), F64 and HP below:

  evaluate / gradient / schur      both arithmetics; the 50-digit side takes every input double exactly
  solve(pb, q, t, X, ...)          double precision: Ceres' TrustRegionMinimizer with the Levenberg-Marquardt strategy and DENSE_SCHUR,
                                   as DESIGN.md §3h restates it (rows marked D / M there: parity with Ceres is NOT pinned)
  polish(pb, q, t, X)              50 digits: Gauss-Newton on the gauge-fixed problem until the step is below 1e-30

The problem, literally (initial_sfm.h:25-63): r = p / |p| - bearing, p = R(q / |q|) X + t, per observation; the rotation of frame l
and the translations of frames l and F - 1 are constant; QuaternionParameterization on the rotations, x [+] d = [cos|d|, sin|d| / |d| d] (x) x.
Tangent Jacobian per observation (checked against a 50-digit derivative of the literal expression by the generator):
N (-2 [R X]x), N, N R with N = (I - ph ph^T) / |p|.  Columns of the reduced camera system: per frame in order, its free rotation (3)
then its free translation (3): 6 F - 9 in all.
"""
import numpy as np

EPS = 2.0 ** -52
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
MIN_DIAG, MAX_DIAG, INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e-6, 1e32, 1e4, 1e16, 1e-32
MIN_RELATIVE_DECREASE, MAX_INVALID = 1e-3, 5
DEFAULTS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)


class F64:
    """double precision"""
    dtype = np.float64
    sqrt, sin, cos = staticmethod(np.sqrt), staticmethod(np.sin), staticmethod(np.cos)

    @staticmethod
    def arr(a):
        return np.array(a, dtype=np.float64)


class _HP:
    """mpmath at hp_ref.DPS digits (imported on first use: the GPU tests never need mpmath)"""
    dtype = object

    def __init__(self):
        self._mp = None

    @property
    def mp(self):
        if self._mp is None:
            import hp_ref  # sets the precision

            self._mp = hp_ref.mp
        return self._mp

    def arr(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a.copy()
        mpf = self.mp.mpf
        return np.array([mpf(float(x)) for x in a.reshape(-1)], dtype=object).reshape(a.shape)

    def sqrt(self, a):
        return np.frompyfunc(self.mp.sqrt, 1, 1)(a)

    def sin(self, a):
        return np.frompyfunc(self.mp.sin, 1, 1)(a)

    def cos(self, a):
        return np.frompyfunc(self.mp.cos, 1, 1)(a)


HP = _HP()


def to_double(a):
    return np.array([float(x) for x in np.asarray(a).reshape(-1)], dtype=np.float64).reshape(np.shape(a))


def problem(F, l, off, frame, bearing):
    """The fixed part of a call: sizes, the CSR, the column map and the pairs of observations of one point."""
    off, frame = np.asarray(off, np.int64), np.asarray(frame, np.int64)
    P, M = len(off) - 1, int(off[-1])
    pt = np.repeat(np.arange(P), np.diff(off))
    col, n = -np.ones((F, 6), np.int64), 0
    for f in range(F):
        if f != l:
            col[f, :3], n = n + np.arange(3), n + 3
        if f != l and f != F - 1:
            col[f, 3:], n = n + np.arange(3), n + 3
    pa, pb_ = [], []
    for i in range(P):
        o = np.arange(off[i], off[i + 1])
        a, b = np.meshgrid(o, o, indexing="ij")
        pa.append(a.reshape(-1)), pb_.append(b.reshape(-1))
    return dict(F=F, l=l, P=P, M=M, off=off, frame=frame, pt=pt, bearing=np.asarray(bearing, np.float64).reshape(M, 3), col=col, n=n,
                pair_a=np.concatenate(pa), pair_b=np.concatenate(pb_), free=col >= 0)


def rotation(q, A):
    """R(q / |q|) for q [F, 4] (w x y z)."""
    n = A.sqrt((q * q).sum(1))
    w, x, y, z = (q / n[:, None]).T
    R = np.empty((len(q), 3, 3), dtype=A.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def mv(Mx, v):
    """[K, 3, 3] x [K, 3] (spelled out: numpy's einsum has no object loop)"""
    return (Mx * v[:, None, :]).sum(2)


def bmm(a, b):
    """[K, i, j] x [K, j, k]"""
    return (a[:, :, :, None] * b[:, None, :, :]).sum(2)


def scatter(idx, vals, size, A):
    out = np.zeros((size,) + vals.shape[1:], dtype=A.dtype)
    if A.dtype == object:
        out = out + A.arr(np.zeros(1))[0]
        for k, i in enumerate(idx):
            out[i] = out[i] + vals[k]
    else:
        np.add.at(out, idx, vals)
    return out


def evaluate(pb, q, t, X, A=F64, jac=True):
    """-> dict(cost, r [M, 3]) and, with jac, Jc [M, 3, 6] (rotation | translation of the observation's frame) and Jp [M, 3, 3]."""
    q, t, X, b = A.arr(q), A.arr(t), A.arr(X), A.arr(pb["bearing"])
    R = rotation(q, A)[pb["frame"]]
    RX = mv(R, X[pb["pt"]])
    p = RX + t[pb["frame"]]
    nrm = A.sqrt((p * p).sum(1))
    ph = p / nrm[:, None]
    r = ph - b
    out = dict(cost=(r * r).sum() / 2, r=r)
    if jac:
        I = np.zeros((1, 3, 3), dtype=A.dtype) + np.eye(3, dtype=np.int64)
        N = (I - ph[:, :, None] * ph[:, None, :]) / nrm[:, None, None]
        S = np.zeros((len(p), 3, 3), dtype=A.dtype)
        S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = 2 * RX[:, 2], -2 * RX[:, 1], -2 * RX[:, 2], 2 * RX[:, 0], 2 * RX[:, 1], -2 * RX[:, 0]
        out["Jc"] = np.concatenate([bmm(N, S), N], axis=2)  # S = -2 [R X]x
        out["Jp"] = bmm(N, R)
    return out


def gradient(pb, ev, A=F64):
    """The tangent gradient J^T r: (gc [F, 6], gp [P, 3]); constant columns are zero."""
    gc = scatter(pb["frame"], (ev["Jc"] * ev["r"][:, :, None]).sum(1), pb["F"], A)
    gp = scatter(pb["pt"], (ev["Jp"] * ev["r"][:, :, None]).sum(1), pb["P"], A)
    return gc * pb["free"], gp


def qmul(a, b):
    w = a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3]
    x = a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2]
    y = a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1]
    z = a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1] + a[:, 3] * b[:, 0]
    return np.stack([w, x, y, z], 1)


def plus(q, t, X, dc, dp, A=F64):
    """x [+] delta: QuaternionParameterization::Plus on the rotations (a zero delta leaves x as it is), sums elsewhere; no renormalisation."""
    q, t, X = A.arr(q), A.arr(t), A.arr(X)
    d = dc[:, :3]
    nd = A.sqrt((d * d).sum(1))
    nz = np.array([bool(v > 0) for v in nd])
    safe = np.where(nz, nd, nd * 0 + 1)
    dq = np.concatenate([A.cos(safe)[:, None], (A.sin(safe) / safe)[:, None] * d], axis=1)
    qn = qmul(dq, q)
    qn[~nz] = q[~nz]
    return qn, t + dc[:, 3:], X + dp


def gradient_max_norm(pb, q, gc, gp, A=F64):
    """max |x - Plus(x, -g)| over the free blocks (TrustRegionMinimizer::EvaluateGradientAndJacobian)."""
    q = A.arr(q)
    qn, _, _ = plus(q, np.zeros((pb["F"], 3)), np.zeros((pb["P"], 3)), -gc, -gp, A)
    vals = [abs(v) for v in (q - qn)[pb["free"][:, 0]].reshape(-1)] + [abs(v) for v in gc[:, 3:][pb["free"][:, 3:]].reshape(-1)] + [abs(v) for v in gp.reshape(-1)]
    return max(vals)


def inv3(V, A):
    """Inverse of symmetric 3 x 3 blocks [K, 3, 3] by the adjugate."""
    a, b, c, d, e, f = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    out = np.empty(V.shape, dtype=A.dtype)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00 / det, c01 / det, c02 / det
    out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = c01 / det, c11 / det, c12 / det
    out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = c02 / det, c12 / det, c22 / det
    return out


def blocks(pb, ev, sc, sp, A=F64):
    """The normal equations of the scaled Jacobian J diag(scale) in blocks: U [F, 6, 6], V [P, 3, 3], W [M, 6, 3], gc [F, 6], gp [P, 3];
    formed unscaled and scaled afterwards, as the device does.  sc [F, 6] (zero on the constant columns), sp [P, 3]."""
    Jc, Jp, fr, pt = ev["Jc"], ev["Jp"], pb["frame"], pb["pt"]
    JcT = np.swapaxes(Jc, 1, 2)
    U = scatter(fr, bmm(JcT, Jc), pb["F"], A) * sc[:, :, None] * sc[:, None, :]
    V = scatter(pt, bmm(np.swapaxes(Jp, 1, 2), Jp), pb["P"], A) * sp[:, :, None] * sp[:, None, :]
    W = bmm(JcT, Jp) * sc[fr][:, :, None] * sp[pt][:, None, :]
    gc = scatter(fr, (Jc * ev["r"][:, :, None]).sum(1), pb["F"], A) * sc
    gp = scatter(pt, (Jp * ev["r"][:, :, None]).sum(1), pb["P"], A) * sp
    return dict(U=U, V=V, W=W, gc=gc, gp=gp)


def jacobi_scale(pb, ev, A=F64):
    """1 / (1 + sqrt(squared column norm)) of the unscaled Jacobian, zero on the constant columns."""
    one = np.ones((pb["F"], 6)) if A is F64 else A.arr(np.ones((pb["F"], 6)))
    onep = np.ones((pb["P"], 3)) if A is F64 else A.arr(np.ones((pb["P"], 3)))
    B = blocks(pb, ev, one, onep, A)
    dU, dV = np.stack([B["U"][:, k, k] for k in range(6)], 1), np.stack([B["V"][:, k, k] for k in range(3)], 1)
    return 1 / (1 + A.sqrt(dU)) * pb["free"], 1 / (1 + A.sqrt(dV))


def clampd(d, A):
    lo, hi = (MIN_DIAG, MAX_DIAG) if A is F64 else (A.mp.mpf(MIN_DIAG), A.mp.mpf(MAX_DIAG))
    return np.where(d < lo, lo, np.where(d > hi, hi, d)) if A is F64 else np.array([min(max(v, lo), hi) for v in d.reshape(-1)], dtype=object).reshape(d.shape)


def schur(pb, B, radius, A=F64, extra_p=None):
    """(S [n, n], rhs [n], Vinv, Dc2, Dp2) of (H + D^2) y = -g with the points eliminated; D^2 = clamp(diag H) / radius (radius None: 0).
    extra_p [P]: added to the diagonal of V (polish() makes a point of one observation definite with it)."""
    F, P, n, col = pb["F"], pb["P"], pb["n"], pb["col"]
    dU, dV = np.stack([B["U"][:, k, k] for k in range(6)], 1), np.stack([B["V"][:, k, k] for k in range(3)], 1)
    Dc2 = clampd(dU, A) / radius if radius is not None else dU * 0
    Dp2 = clampd(dV, A) / radius if radius is not None else dV * 0
    if extra_p is not None:
        Dp2 = Dp2 + extra_p[:, None]
    V = B["V"].copy()
    for k in range(3):
        V[:, k, k] = V[:, k, k] + Dp2[:, k]
    Vinv = inv3(V, A)
    Y = bmm(B["W"], Vinv[pb["pt"]])  # [M, 6, 3]
    S6 = np.zeros((F, F, 6, 6), dtype=A.dtype)
    for f in range(F):
        S6[f, f] = B["U"][f]
        for k in range(6):
            S6[f, f, k, k] = S6[f, f, k, k] + Dc2[f, k]
    pa, pb_ = pb["pair_a"], pb["pair_b"]
    E = bmm(Y[pa], np.swapaxes(B["W"][pb_], 1, 2))  # [pairs, 6, 6]
    S6 = S6.reshape(F * F, 6, 6) - scatter(pb["frame"][pa] * F + pb["frame"][pb_], E, F * F, A)
    S6 = S6.reshape(F, F, 6, 6)
    rc = -B["gc"] + scatter(pb["frame"], (Y * B["gp"][pb["pt"]][:, None, :]).sum(2), F, A)
    fr, k6 = np.nonzero(col >= 0)
    S = np.array([[S6[fr[a], fr[b], k6[a], k6[b]] for b in range(n)] for a in range(n)], dtype=A.dtype).reshape(n, n)
    return dict(S=S, rhs=rc[fr, k6], Vinv=Vinv, fr=fr, k6=k6, Dc2=Dc2, Dp2=Dp2)


def back_substitute(pb, B, sch, yc_flat, A=F64):
    """yc [F, 6] (zeros on the constant columns) and yp [P, 3] = Vinv (-gp - sum W^T yc)."""
    yc = np.zeros((pb["F"], 6), dtype=A.dtype)
    if A.dtype == object:
        yc = yc + A.arr(np.zeros(1))[0]
    yc[sch["fr"], sch["k6"]] = yc_flat
    wy = scatter(pb["pt"], (B["W"] * yc[pb["frame"]][:, :, None]).sum(1), pb["P"], A)
    return yc, mv(sch["Vinv"], -B["gp"] - wy)


def xnorm(pb, q, t, X):
    return float(np.sqrt((q[pb["free"][:, 0]] ** 2).sum() + (t[pb["free"][:, 3]] ** 2).sum() + (X ** 2).sum()))


def solve(pb, q, t, X, max_num_iterations=-1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0):
    """lfvio_sfm_ba in double precision.  Tolerances <= 0 and max_num_iterations < 0 take Ceres' defaults; max_num_iterations = 0 is
    iteration 0 alone (the evaluation at the start)."""
    opt = dict(DEFAULTS)
    for k, v in (("function_tolerance", function_tolerance), ("gradient_tolerance", gradient_tolerance), ("parameter_tolerance", parameter_tolerance)):
        if v > 0:
            opt[k] = v
    max_it = opt["max_num_iterations"] if max_num_iterations < 0 else max_num_iterations
    q, t, X = np.array(q, np.float64), np.array(t, np.float64), np.array(X, np.float64)
    with np.errstate(all="ignore"):
        return _solve(pb, q, t, X, max_it, opt)


def _solve(pb, q, t, X, max_it, opt):
    F, P = pb["F"], pb["P"]
    ev = evaluate(pb, q, t, X)
    x_cost = float(ev["cost"])
    if not np.isfinite(x_cost):
        return dict(rc=-3)
    sc, sp = jacobi_scale(pb, ev)
    gc, gp = gradient(pb, ev)
    x_norm = xnorm(pb, q, t, X)
    radius, factor = INITIAL_RADIUS, 2.0
    it = dict(cost=x_cost, cost_change=0.0, gradient_max_norm=float(gradient_max_norm(pb, q, gc, gp)), step_norm=0.0, relative_decrease=0.0,
              step_is_valid=0, step_is_successful=0)
    trace, n_succ, n_unsucc, n_invalid, iteration, term = [], 0, 0, 0, 0, NO_CONVERGENCE
    initial_cost = x_cost
    B, end = None, None  # end: the test that ended the run on a step that is not pushed, and the ratio it compared
    while True:
        if it["step_is_successful"]:
            n_succ += 1
        else:
            n_unsucc += 1
        it["trust_region_radius"] = radius
        trace.append(it)
        if iteration >= max_it:
            term = NO_CONVERGENCE
            break
        if it["step_is_successful"] and it["gradient_max_norm"] <= opt["gradient_tolerance"]:
            term = CONVERGENCE
            break
        if radius <= MIN_RADIUS:
            term = CONVERGENCE
            break
        it = dict(cost=x_cost, cost_change=0.0, gradient_max_norm=0.0, step_norm=0.0, relative_decrease=0.0, step_is_valid=0, step_is_successful=0)
        iteration += 1
        # LevenbergMarquardtStrategy::ComputeStep on the scaled Jacobian, DENSE_SCHUR
        if B is None:
            B = blocks(pb, ev, sc, sp)
        sch = schur(pb, B, radius)
        valid = False
        try:
            L = np.linalg.cholesky(sch["S"]) if np.all(np.isfinite(sch["S"])) else None
        except np.linalg.LinAlgError:
            L = None
        if L is not None:
            z = np.linalg.solve(L, sch["rhs"])
            yc, yp = back_substitute(pb, B, sch, np.linalg.solve(L.T, z))
            dc, dp = yc * sc, yp * sp
            if np.all(np.isfinite(dc)) and np.all(np.isfinite(dp)):
                Jd = (ev["Jc"] * dc[pb["frame"]][:, None, :]).sum(2) + (ev["Jp"] * dp[pb["pt"]][:, None, :]).sum(2)
                model_cost_change = float(-(Jd * (ev["r"] + Jd / 2)).sum())
                valid = model_cost_change > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            n_invalid += 1
            if n_invalid >= MAX_INVALID:
                term = FAILURE
                break
            radius, factor = radius / factor, 2.0 * factor  # StepIsInvalid = StepRejected
            continue
        n_invalid = 0
        qc, tc, Xc = plus(q, t, X, dc, dp)
        evc = evaluate(pb, qc, tc, Xc, jac=False)
        cand_cost = float(evc["cost"]) if np.isfinite(evc["cost"]) else np.finfo(np.float64).max
        fr0, fr3 = pb["free"][:, 0], pb["free"][:, 3]
        it["step_norm"] = float(np.sqrt(((q - qc)[fr0] ** 2).sum() + ((t - tc)[fr3] ** 2).sum() + ((X - Xc) ** 2).sum()))
        if it["step_norm"] <= opt["parameter_tolerance"] * (x_norm + opt["parameter_tolerance"]):
            term, end = CONVERGENCE, dict(test="parameter", ratio=it["step_norm"] / (x_norm + opt["parameter_tolerance"]))
            break
        it["cost_change"] = x_cost - cand_cost
        if abs(it["cost_change"]) <= opt["function_tolerance"] * x_cost:
            term, end = CONVERGENCE, dict(test="function", ratio=abs(it["cost_change"]) / x_cost)
            break
        it["relative_decrease"] = it["cost_change"] / model_cost_change
        if it["relative_decrease"] > MIN_RELATIVE_DECREASE:
            q, t, X = qc, tc, Xc
            x_norm = xnorm(pb, q, t, X)
            ev = evaluate(pb, q, t, X)
            x_cost = float(ev["cost"])
            B = None
            gc, gp = gradient(pb, ev)
            it["cost"], it["gradient_max_norm"], it["step_is_successful"] = x_cost, float(gradient_max_norm(pb, q, gc, gp)), 1
            rho = it["relative_decrease"]
            radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            factor = 2.0
        else:
            it["cost"] = cand_cost
            radius, factor = radius / factor, 2.0 * factor
    Q, T = drop_in(q, t)
    return dict(rc=0, c_rotation=q, c_translation=t, position=X, termination=term, num_iterations=len(trace), num_successful_steps=n_succ,
                num_unsuccessful_steps=n_unsucc, initial_cost=initial_cost, final_cost=x_cost,
                accepted=int(term == CONVERGENCE or x_cost < 5e-3), Q=Q, T=T, trace=trace, end=end)


def drop_in(q, t, A=F64):
    """initial_sfm.cpp:295-309: Q = q.inverse() (conjugate / squared norm), T = -(Q * t) (Eigen's _transformVector)."""
    q, t = A.arr(q), A.arr(t)
    n2 = (q * q).sum(1)
    Q = np.concatenate([q[:, :1], -q[:, 1:]], 1) / n2[:, None]
    u = Q[:, 1:]
    cr = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    uv = cr(u, t)
    uv = uv + uv
    return Q, -(t + Q[:, :1] * uv + cr(u, uv))


def gauss_newton_step(pb, q, t, X, A=F64, active_c=None, single=None):
    """The undamped Gauss-Newton step of the gauge-fixed problem at (q, t, X): (dc [F, 6], dp [P, 3]).  active_c [F, 6]: columns
    that take part (a frame with no observation has none); single [P]: points of one observation, whose depth the problem
    does not determine, get 1e-12 on their diagonal (a stationary point is a stationary point under any damping)."""
    ev = evaluate(pb, q, t, X, A)
    act = pb["free"] if active_c is None else (pb["free"] & active_c)
    one, onep = A.arr(act.astype(np.float64)), A.arr(np.ones((pb["P"], 3)))
    B = blocks(pb, ev, one, onep, A)
    extra = None if single is None else A.arr(np.where(single, 1e-12, 0.0))
    sch = schur(pb, B, None, A, extra)
    S, rhs = sch["S"].copy(), sch["rhs"]
    dead = ~act[sch["fr"], sch["k6"]]
    for k in np.nonzero(dead)[0]:
        S[k, k] = S[k, k] + 1
    if A is F64:
        y = np.linalg.solve(S, rhs)
    else:
        y = np.array(list(A.mp.cholesky_solve(A.mp.matrix(S.tolist()), A.mp.matrix(rhs.tolist()))), dtype=object)
    return back_substitute(pb, B, sch, y, A)


def polish(pb, q, t, X, active_c=None, single=None, tol=1e-30, max_steps=250, log=None):
    """50 digits: Gauss-Newton from (q, t, X) until the largest |step| is below tol.  Returns mpmath arrays."""
    A = HP
    q, t, X = A.arr(q), A.arr(t), A.arr(X)
    for k in range(max_steps):
        dc, dp = gauss_newton_step(pb, q, t, X, A, active_c, single)
        step = max(max(abs(v) for v in dc.reshape(-1)), max(abs(v) for v in dp.reshape(-1)))
        q, t, X = plus(q, t, X, dc, dp, A)
        if log:
            log(f"    polish {k}: step {float(step):.3e}")
        if step < tol:
            return q, t, X
    raise RuntimeError("polish: no convergence")


def dense_jacobian(pb, ev):
    """J [3 M, n + 3 P] (double), free columns only, for condition numbers and scipy."""
    M, n, P = pb["M"], pb["n"], pb["P"]
    J = np.zeros((3 * M, n + 3 * P))
    for o in range(M):
        f, i = pb["frame"][o], pb["pt"][o]
        for k in range(6):
            if pb["col"][f, k] >= 0:
                J[3 * o:3 * o + 3, pb["col"][f, k]] = ev["Jc"][o][:, k]
        J[3 * o:3 * o + 3, n + 3 * i:n + 3 * i + 3] = ev["Jp"][o]
    return J
