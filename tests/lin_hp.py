"""50-digit statement of the residual-and-Jacobian sweep of optimization() (test infrastructure: mpmath and numpy), the reference that
tests/test_lin_hp.py holds k_lin, k_imu_raw, k_linw, k_linb and k_setup's information roots to, block by block.

Written from the reference's formulas, line by line — not from tests/np_ref.py's code and not from the kernels:

  visual factor      factor/projection_td_factor.cpp:20-32 (rows, tangent base with its `a == (0,0,1)` branch), :54-75 (the chain with
                     Quaternion::inverse() = conjugate / |q|^2, residual on the unit sphere), :79-146 (toRotationMatrix() and its
                     transposes in the Jacobians, the td column as coded at :143-144); without td factor/projection_factor.cpp:35-49
  IMU factor         factor/integration_base.h:160-186 (evaluate), factor/imu_factor.h:64-66 (sqrt_info = LLT(P^-1).matrixL()^T),
                     :72-196 (Jacobians in the tangent), utility/utility.h:16-28, :41-64 (deltaQ, positify = identity, Qleft, Qright)
  loss and corrector estimator.cpp:681 (CauchyLoss(1.0)), restated in the reference at factor/marginalization_factor.cpp:37-68
  prior              factor/marginalization_factor.cpp:343-377 (r0 + J0 dx with the sign branch of the quaternion difference)
  assembly           estimator.cpp:690-703 (constant ex / td), :713 (prior, no loss), :718-725 (IMU factors, `sum_dt > 10.0` skipped, no
                     loss), :729-771 (one visual factor per observation after a landmark's first, Cauchy loss); tangent columns through
                     factor/pose_local_parameterization.cpp:3-27 (the Jacobian's first six columns ARE the tangent's)

For CauchyLoss rho'' = -1 / (1 + s)^2 <= 0 always, so the `alpha` branch of the corrector (marginalization_factor.cpp:54-60) is dead.  It
is stated anyway (cauchy) and ALPHA_TAKEN counts how often it was taken: the tests assert zero.

Every input is a double of an abi.Window and is taken exactly; nothing is rounded on the way.  mpmath numbers travel in numpy object
arrays; the quaternion and rotation helpers are those of tests/hp_ref.py.  A Statement keeps every result as an unevaluated pair of
doubles (hi + lo, 32 digits: the difference to a double-precision result is then formed in numpy) and, for every sum, the sum of the
absolute values of its terms (a double: it is a unit, three digits suffice) — the unit the Schur sums of tests/solve_hp.py use.

Units.  A deviation is reported in eps x the unit of its block: the largest sum of absolute terms among the block's entries.  A term is
a product of Jacobian (and residual) entries, and an entry is itself the end of a chain that cancels (the IMU residual: 0.5 g dt^2 + Pj -
Pi - Vi dt against delta_p; the visual chain: Xw - Pj, then two unit vectors against each other).  So every factor returns, beside r
and J, their own units abs_r and abs_J — the same expressions with the absolute value of every term — and a product enters a sum's
unit by first-order propagation (product_unit below).  The IMU factor is weighted by sqrt_info, the transposed Cholesky factor of the INVERSE of the covariance
(kappa_2(P) = 1e4 for the pre-integrations of lfvio.synth).  Measured on the comparators: in the assembled blocks, the gradient and the
cost of a factor — whose unit is the largest sum of a 6- or 9-wide block — their figures are O(1 - 100) as they stand, so those units
carry no conditioning factor.  The 3 x 3 blocks of a factor's 30 x 30 source are another matter: the error of a double-precision
sqrt_info is eps kappa_2(P) of its LARGEST entries, and a 3 x 3 block made of its small ones (position rows against bias columns) is
1e3 .. 1e4 eps of its own unit in both comparators; that metric's unit is eps kappa_2(P)^IMU_COND_POWER x the block's unit,
IMU_COND_POWER = 1, which puts the comparators at 0.1 - 1.1 (as tests/test_feature_hp.py does with eps sigma_1 / sigma_4).

The bars at the end of the file are 16 x the worst figure of two double-precision comparators (tests/np_ref.py and oracle/) over the case
list of tests/lin_cases.py, per metric and case class — measured on the CPU (tests/test_lin_hp_ref.py), never on a device.
"""
import mpmath as mp
import numpy as np

import hp_ref
import np_ref

DPS = 50
mp.mp.dps = DPS
KC, KP = np_ref.KC, np_ref.KP
EPS = 2.0 ** -53
CERTIFICATE = 1e-40
ALPHA_TAKEN = [0]
# The power of kappa_2(P) in the unit of the 3 x 3 blocks of an IMU factor's source (metric imu33; see above): with 0 the comparators
# sit at 1e3 .. 1e4, with 1 at 0.1 .. 1.1.
IMU_COND_POWER = 1.0


# ------------------------------------------------------------------------------------------------------------------------
# small helpers on object arrays
# ------------------------------------------------------------------------------------------------------------------------
def to_mp(a):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.size, dtype=object)
    for i, v in enumerate(a.ravel()):
        out[i] = mp.mpf(float(v))
    return out.reshape(a.shape)


def to_f(a):
    a = np.asarray(a, dtype=object)
    return np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def split(a):
    """(hi, lo) doubles with hi + lo = a to 32 digits."""
    a = np.asarray(a, dtype=object)
    hi = to_f(a)
    lo = np.array([float(v - mp.mpf(float(h))) for v, h in zip(a.ravel(), hi.ravel())], dtype=np.float64).reshape(a.shape)
    return hi, lo


def _arr(x):
    return np.array(list(x), dtype=object)


def _R(q):
    return np.array(hp_ref.q_to_R(list(q)).tolist(), dtype=object)


def _rot(q, v):
    return _arr(hp_ref.q_rot(list(q), list(v)))


def _qmul(a, b):
    return _arr(hp_ref.qmul(list(a), list(b)))


def _skew(v):
    return np.array(hp_ref.skew(list(v)).tolist(), dtype=object)


def _qinv(q):
    """Eigen's Quaternion::inverse(): conjugate / squared norm."""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return _arr([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2])


def _norm(v):
    return mp.sqrt(mp.fsum(x * x for x in v))


def _pose_q(p):
    return _arr([p[6], p[3], p[4], p[5]])


def _Qleft(q):
    L = np.empty((4, 4), dtype=object)
    L[0, 0] = q[0]
    L[0, 1:] = -q[1:]
    L[1:, 0] = q[1:]
    L[1:, 1:] = q[0] * _eye(3) + _skew(q[1:])
    return L


def _Qright(p):
    Rm = np.empty((4, 4), dtype=object)
    Rm[0, 0] = p[0]
    Rm[0, 1:] = -p[1:]
    Rm[1:, 0] = p[1:]
    Rm[1:, 1:] = p[0] * _eye(3) - _skew(p[1:])
    return Rm


def _eye(n):
    E = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            E[i, j] = mp.mpf(1 if i == j else 0)
    return E


def _zeros(*shape):
    Z = np.empty(shape, dtype=object)
    Z.fill(mp.mpf(0))
    return Z


def _deltaQ(theta):
    return _arr([mp.mpf(1), theta[0] / 2, theta[1] / 2, theta[2] / 2])


# ------------------------------------------------------------------------------------------------------------------------
# the visual factor
# ------------------------------------------------------------------------------------------------------------------------
def tangent_base(pts_j):
    """projection_td_factor.cpp:25-32.  The comparison `a == tmp` is exact in the reference (doubles) and exact here: a normalized
    vector is (0, 0, 1) in either arithmetic exactly when x = y = 0 and z > 0.  Returns (B [2, 3], branch taken)."""
    n = _norm(pts_j)
    a = _arr([c / n for c in pts_j])
    tmp = _arr([mp.mpf(0), mp.mpf(0), mp.mpf(1)])
    branch = bool(pts_j[0] == 0 and pts_j[1] == 0 and pts_j[2] > 0)
    if branch:
        tmp = _arr([mp.mpf(1), mp.mpf(0), mp.mpf(0)])
    d = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2]
    b1 = tmp - a * d
    b1 = b1 / _norm(b1)
    b2 = _arr(hp_ref.cross(list(a), list(b1)))
    return np.stack([b1, b2]), branch


def visual(use_td, TR, ROW, s, pts_i, pts_j, vel_i, vel_j, td_i, td_j, uvy_i, uvy_j, pose_i, pose_j, ex, lam, td, td_true=False,
           want_J=True):
    """One ProjectionTdFactor (use_td) / ProjectionFactor.  All arguments mpf / object arrays.  Returns r [2], J [2, 20] over
    [pose_i (6) | pose_j (6) | ex (6) | td | lambda] in the tangent, and the units abs_r [2], abs_J [2, 20] (doubles): the same expressions
    with the absolute value of every term of every step, times gamma = max |terms of Xcj| / |Xcj| (the chain ends in Xw - Pj and in
    a direction; every entry of r and J inherits what that has cancelled).
    td_true: the td column as the derivative of the residual (np_ref.TD_TRUE_DERIVATIVE names the difference: the reference's second
    term is sqrt_info velocity_j.head(2), not sqrt_info B d(pj / |pj|) / d pj velocity_j)."""
    B, _ = tangent_base(pts_j)
    Pi, Qi, Pj, Qj, tic, qic = pose_i[:3], _pose_q(pose_i), pose_j[:3], _pose_q(pose_j), ex[:3], _pose_q(ex)
    if use_td:
        row_i, row_j = uvy_i - ROW / 2, uvy_j - ROW / 2
        pi = pts_i - (td - td_i + TR / ROW * row_i) * vel_i
        pj = pts_j - (td - td_j + TR / ROW * row_j) * vel_j
    else:
        pi, pj = pts_i, pts_j
    Xci = pi / lam
    Xbi = _rot(qic, Xci) + tic
    Xw = _rot(Qi, Xbi) + Pi
    Xbj = _rot(_qinv(Qj), Xw - Pj)
    Xcj = _rot(_qinv(qic), Xbj - tic)
    n, m = _norm(Xcj), _norm(pj)
    u, v = Xcj / n, pj / m
    r = s * B.dot(u - v)
    # ---- what the chain cancels from, in double (units): |.| of every term of every step; gamma = how far its end has cancelled
    f = lambda x: np.abs(to_f(x))  # noqa: E731
    sf, lamf, nf = float(s), abs(float(lam)), float(n)
    aB, aRi, aRjT, aric, aricT = f(B), f(_R(Qi)), f(_R(_qinv(Qj))), f(_R(qic)), f(_R(_qinv(qic)))
    aXci = f(Xci)
    aXbi = aric @ aXci + f(tic)
    aXw = aRi @ aXbi + f(Pi)
    aXbj = aRjT @ (aXw + f(Pj))
    aXcj = aricT @ (aXbj + f(tic))
    gamma = float(aXcj.max()) / nf
    abs_r = gamma * sf * (aB @ (f(u) + f(v)))
    if not want_J:
        return r, None, abs_r, None
    Ri, Rj, ric = _R(Qi), _R(Qj), _R(qic)
    n3 = n * n * n
    nj = _eye(3) / n - np.outer(Xcj, Xcj) / n3
    red = s * B.dot(nj)
    A = ric.T.dot(Rj.T)          # ric^T Rj^T
    ARi = A.dot(Ri)
    T = ARi.dot(ric)
    J = _zeros(2, 20)
    J[:, 0:3] = red.dot(A)
    J[:, 3:6] = red.dot(ARi.dot(-_skew(Xbi)))
    J[:, 6:9] = red.dot(-A)
    J[:, 9:12] = red.dot(ric.T.dot(_skew(Xbj)))
    J[:, 12:15] = red.dot(ric.T.dot(Rj.T.dot(Ri) - _eye(3)))
    TX = T.dot(Xci)
    J[:, 15:18] = red.dot(-T.dot(_skew(Xci)) + _skew(TX) + _skew(ric.T.dot(Rj.T.dot(Ri.dot(tic) + Pi - Pj) - tic)))
    if use_td:
        first = red.dot(T.dot(vel_i)) / lam * -1
        if td_true:
            m3 = m * m * m
            J[:, 18] = first + s * B.dot((_eye(3) / m - np.outer(pj, pj) / m3).dot(vel_j))
        else:
            J[:, 18] = first + s * vel_j[:2]
    J[:, 19] = red.dot(T.dot(pi)) * -1 / (lam * lam)
    ask = lambda x: np.abs(np_ref.skew(x))  # noqa: E731
    aricT_, aRjT_ = f(ric.T), f(Rj.T)
    ared = gamma * sf * (aB @ (np.eye(3) / nf + np.outer(f(Xcj), f(Xcj)) / nf ** 3))
    aA = aricT_ @ aRjT_
    aARi = aA @ aRi
    aT = aARi @ aric
    abs_J = np.zeros((2, 20))
    abs_J[:, 0:3] = abs_J[:, 6:9] = ared @ aA
    abs_J[:, 3:6] = ared @ (aARi @ ask(aXbi))
    abs_J[:, 9:12] = ared @ (aricT_ @ ask(aXbj))
    abs_J[:, 12:15] = ared @ (aricT_ @ (aRjT_ @ aRi + np.eye(3)))
    abs_J[:, 15:18] = ared @ (aT @ ask(aXci) + ask(aT @ aXci) + ask(aricT_ @ (aRjT_ @ (aRi @ f(tic) + f(Pi) + f(Pj)) + f(tic))))
    if use_td:
        abs_J[:, 18] = ared @ (aT @ f(vel_i)) / lamf + sf * f(vel_j)[:2]
    abs_J[:, 19] = ared @ (aT @ f(pi)) / (lamf * lamf)
    return r, J, abs_r, abs_J


# ------------------------------------------------------------------------------------------------------------------------
# the IMU factor
# ------------------------------------------------------------------------------------------------------------------------
def cholesky_lower(A):
    n = A.shape[0]
    L = _zeros(n, n)
    for j in range(n):
        d = A[j, j] - mp.fsum(L[j, k] * L[j, k] for k in range(j))
        assert d > 0, f"cholesky_lower: pivot {j}"
        L[j, j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - mp.fsum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    return L


def inverse(P):
    """P^-1 of the 15 x 15 doubles as they stand (a stored covariance is symmetric to rounding only, and Eigen's inverse() reads all of it):
    mpmath's LU with partial pivoting."""
    n = P.shape[0]
    Pi = mp.matrix(P.tolist()) ** -1
    return np.array([[Pi[i, j] for j in range(n)] for i in range(n)], dtype=object)


def sqrt_info(P):
    """imu_factor.h:64: LLT(P^-1).matrixL().transpose(); LLT reads the lower triangle of its argument."""
    return cholesky_lower(inverse(P)).T


def pre_fields(pre):
    """The doubles of one abi.Preintegration, exactly.  delta_q comes as x y z w."""
    J = to_mp(np.array(pre.jacobian[:]).reshape(15, 15))
    P = to_mp(np.array(pre.covariance[:]).reshape(15, 15))
    q = pre.delta_q
    return dict(sum_dt=mp.mpf(float(pre.sum_dt)), dp=to_mp(pre.delta_p[:]), dq=to_mp([q[3], q[0], q[1], q[2]]), dv=to_mp(pre.delta_v[:]),
                ba=to_mp(pre.linearized_ba[:]), bg=to_mp(pre.linearized_bg[:]), J=J, P=P)


def imu_raw(f, G, pose_i, sb_i, pose_j, sb_j, want_J=True, exact_rotation=False):
    """Unweighted residual [15] and Jacobian [15, 30] over [pose_i (6) | sb_i (9) | pose_j (6) | sb_j (9)], and abs_r [15], abs_J
    [15, 30] (mpf: what every entry cancels from).  f: pre_fields' dict (dq may be any mpf quaternion).
    exact_rotation: the three rotation-row blocks as the derivative of the residual instead of the reference's expressions.  The
    reference's (imu_factor.h:100, :132, :166) equal the derivative where corrected_delta_q is a unit quaternion and Bgi =
    linearized_bg; deltaQ leaves |corrected_delta_q|^2 = 1 + |dq_dbg dbg|^2 / 4, and :132 is the derivative at dbg = 0."""
    Pi, Qi, Pj, Qj = pose_i[:3], _pose_q(pose_i), pose_j[:3], _pose_q(pose_j)
    Vi, Bai, Bgi, Vj, Baj, Bgj = sb_i[:3], sb_i[3:6], sb_i[6:9], sb_j[:3], sb_j[3:6], sb_j[6:9]
    Jm, dt = f["J"], f["sum_dt"]
    dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg = Jm[0:3, 9:12], Jm[0:3, 12:15], Jm[3:6, 12:15], Jm[6:9, 9:12], Jm[6:9, 12:15]
    dba, dbg = Bai - f["ba"], Bgi - f["bg"]
    cq = _qmul(f["dq"], _deltaQ(dq_dbg.dot(dbg)))
    cv = f["dv"] + dv_dba.dot(dba) + dv_dbg.dot(dbg)
    cp = f["dp"] + dp_dba.dot(dba) + dp_dbg.dot(dbg)
    Qi_inv = _qinv(Qi)
    half = mp.mpf(1) / 2
    vp = half * G * dt * dt + Pj - Pi - Vi * dt
    vv = G * dt + Vj - Vi
    rp, rv = _rot(Qi_inv, vp), _rot(Qi_inv, vv)
    r = _zeros(15)
    r[0:3] = rp - cp
    r[3:6] = 2 * _qmul(_qinv(cq), _qmul(Qi_inv, Qj))[1:]
    r[6:9] = rv - cv
    r[9:12] = Baj - Bai
    r[12:15] = Bgj - Bgi
    RiT = _R(Qi_inv)
    aR = np.abs(RiT)
    abs_r = _zeros(15)
    abs_r[0:3] = aR.dot(np.abs(half * G * dt * dt) + np.abs(Pj) + np.abs(Pi) + np.abs(Vi * dt)) + np.abs(f["dp"]) + np.abs(dp_dba).dot(np.abs(dba)) + np.abs(dp_dbg).dot(np.abs(dbg))
    ci, bq = _qinv(cq), _qmul(Qi_inv, Qj)  # (the vector part of a product of near-unit quaternions: four terms each, which cancel)
    abs_r[3:6] = 2 * _arr([abs(ci[0] * bq[1]) + abs(ci[1] * bq[0]) + abs(ci[2] * bq[3]) + abs(ci[3] * bq[2]),
                           abs(ci[0] * bq[2]) + abs(ci[2] * bq[0]) + abs(ci[3] * bq[1]) + abs(ci[1] * bq[3]),
                           abs(ci[0] * bq[3]) + abs(ci[3] * bq[0]) + abs(ci[1] * bq[2]) + abs(ci[2] * bq[1])])
    abs_r[6:9] = aR.dot(np.abs(G * dt) + np.abs(Vj) + np.abs(Vi)) + np.abs(f["dv"]) + np.abs(dv_dba).dot(np.abs(dba)) + np.abs(dv_dbg).dot(np.abs(dbg))
    abs_r[9:12] = np.abs(Baj) + np.abs(Bai)
    abs_r[12:15] = np.abs(Bgj) + np.abs(Bgi)
    if not want_J:
        return r, None, abs_r, None
    J = _zeros(15, 30)
    I3 = _eye(3)
    # pose_i
    J[0:3, 0:3] = -RiT
    J[0:3, 3:6] = _skew(rp)
    QjiL = _qmul(_qinv(Qj), Qi)
    if exact_rotation:
        J[3:6, 3:6] = -(_Qleft(_qinv(cq)).dot(_Qright(_qmul(Qi_inv, Qj))))[1:, 1:]
    else:
        J[3:6, 3:6] = -(_Qleft(QjiL).dot(_Qright(cq)))[1:, 1:]
    J[6:9, 3:6] = _skew(rv)
    # speed / bias i
    J[0:3, 6:9] = -RiT * dt
    J[0:3, 9:12] = -dp_dba
    J[0:3, 12:15] = -dp_dbg
    if exact_rotation:
        # r = 2 vec(cq^-1 b), cq^-1 = conj(cq) / |cq|^2, cq = dq (1, phi / 2), phi = dq_dbg dbg
        b = _qmul(Qi_inv, Qj)
        n2 = mp.fsum(c * c for c in cq)
        conj = _arr([cq[0], -cq[1], -cq[2], -cq[3]])
        D = _zeros(3, 3)
        for k in range(3):
            e = _zeros(4)
            e[1 + k] = half  # d (1, phi / 2) / d phi_k
            dcq = _qmul(f["dq"], e)
            dconj = _arr([dcq[0], -dcq[1], -dcq[2], -dcq[3]])
            dn2 = 2 * mp.fsum(cq[c] * dcq[c] for c in range(4))
            dinv = dconj / n2 - conj * dn2 / (n2 * n2)
            D[:, k] = 2 * _qmul(dinv, b)[1:]
        J[3:6, 12:15] = D.dot(dq_dbg)
    else:
        J[3:6, 12:15] = -(_Qleft(_qmul(QjiL, f["dq"]))[1:, 1:]).dot(dq_dbg)
    J[6:9, 6:9] = -RiT
    J[6:9, 9:12] = -dv_dba
    J[6:9, 12:15] = -dv_dbg
    J[9:12, 9:12] = -I3
    J[12:15, 12:15] = -I3
    # pose_j
    J[0:3, 15:18] = RiT
    if exact_rotation:
        J[3:6, 18:21] = (_Qleft(_qmul(_qinv(cq), _qmul(Qi_inv, Qj))))[1:, 1:]
    else:
        J[3:6, 18:21] = _Qleft(_qmul(_qmul(_qinv(cq), Qi_inv), Qj))[1:, 1:]
    # speed / bias j
    J[6:9, 21:24] = RiT
    J[9:12, 24:27] = I3
    J[12:15, 27:30] = I3
    abs_J = np.abs(J)  # (entries that are a rotated difference enter with what the difference cancels from)
    abs_J[0:3, 3:6] = np.abs(_skew(aR.dot(np.abs(half * G * dt * dt) + np.abs(Pj) + np.abs(Pi) + np.abs(Vi * dt))))
    abs_J[6:9, 3:6] = np.abs(_skew(aR.dot(np.abs(G * dt) + np.abs(Vj) + np.abs(Vi))))
    return r, J, abs_r, abs_J


def imu(pre, G, pose_i, sb_i, pose_j, sb_j, want_J=True):
    """One IMUFactor, weighted: r [15], J [15, 30], abs_r [15], abs_J [15, 30] (|sqrt_info| |.|: the weighting is a sum too), kappa_2(P)."""
    f = pre_fields(pre)
    r, J, abs_r, abs_J = imu_raw(f, G, pose_i, sb_i, pose_j, sb_j, want_J)
    S = sqrt_info(f["P"])
    aS = np.abs(S)
    sv = np.linalg.svd(to_f(f["P"]), compute_uv=False)
    return S.dot(r), (S.dot(J) if want_J else None), aS.dot(abs_r), (aS.dot(abs_J) if want_J else None), float(sv[0] / sv[-1])


# ------------------------------------------------------------------------------------------------------------------------
# loss, prior
# ------------------------------------------------------------------------------------------------------------------------
def cauchy(r, J):
    """CauchyLoss(1.0) and Ceres' Corrector on one residual block: rho0, scaled r, corrected J, sqrt(rho')."""
    s = mp.fsum(x * x for x in r)
    rho0 = mp.log(1 + s)
    rho1 = 1 / (1 + s)
    rho2 = -rho1 * rho1
    sq = mp.sqrt(rho1)
    if s == 0 or rho2 <= 0:
        return rho0, sq * r, (sq * J if J is not None else None), sq
    ALPHA_TAKEN[0] += 1  # dead for this loss: rho2 < 0 for every s
    D = 1 + 2 * s * rho2 / rho1
    alpha = 1 - mp.sqrt(D)
    Jc = None if J is None else sq * (J - alpha / s * np.outer(r, r.dot(J)))
    return rho0, sq / (1 - alpha) * r, Jc, sq


def prior_dx(prior, st):
    """dx [n] of marginalization_factor.cpp:346-363 and, per quaternion block, whether the `w >= 0` test failed (the sign branch)."""
    n = prior.n
    dx = _zeros(n)
    flipped = []
    for i in range(prior.num_blocks):
        kind, frame, idx = prior.blocks[i].kind, prior.blocks[i].frame, prior.block_idx[i]
        x0 = to_mp(np.array(prior.block_x0[i][:]))
        x = st.block(kind, frame)
        if kind in (0, 2):
            dx[idx:idx + 3] = x[:3] - x0[:3]
            dq = _qmul(_qinv(_pose_q(x0)), _pose_q(x))
            v = 2 * dq[1:]
            if not dq[0] >= 0:
                v = -v
                flipped.append(i)
            dx[idx + 3:idx + 6] = v
        else:
            sz = 9 if kind == 1 else 1
            dx[idx:idx + sz] = x[:sz] - x0[:sz]
    return dx, flipped


class State:
    """The state of a window as mpf: pose [11, 7], sb [11, 9], ex [7], td, lam [N]."""

    def __init__(self, w):
        self.pose, self.sb, self.ex = to_mp(w.pose), to_mp(w.speed_bias), to_mp(w.ex_pose)
        self.td, self.lam = mp.mpf(float(w.td)), to_mp(w.inv_depth)

    def block(self, kind, frame):
        return (self.pose[frame], self.sb[frame], self.ex, _arr([self.td]))[kind]


# ------------------------------------------------------------------------------------------------------------------------
# assembly
# ------------------------------------------------------------------------------------------------------------------------
BLOCKS = [("pose", f, 6 * f, 6) for f in range(11)] + [("ex", 0, 66, 6), ("td", 0, 72, 1)] + [("sb", f, 73 + 9 * f, 9) for f in range(11)]
CAMERA_BLOCKS = BLOCKS[:13]


def imu_columns(f):
    return list(range(6 * f, 6 * f + 6)) + list(range(73 + 9 * f, 82 + 9 * f)) + list(range(6 * f + 6, 6 * f + 12)) + list(range(82 + 9 * f, 91 + 9 * f))


def prior_columns(prior):
    """prior column -> tangent column (-1 is never left)."""
    cmap = np.full(prior.n, -1, dtype=np.int64)
    for i in range(prior.num_blocks):
        kind, frame, idx = prior.blocks[i].kind, prior.blocks[i].frame, prior.block_idx[i]
        for k in range(np_ref.block_local(kind)):
            cmap[idx + k] = np_ref.block_off(kind, frame) + k
    assert (cmap >= 0).all() and len(set(cmap.tolist())) == prior.n
    return cmap


def observations(w):
    """(landmark, first observation, this observation, frame i, frame j) of every visual factor, in the reference's order."""
    for l in range(w.N):
        o0, o1, fi = int(w.obs_offset[l]), int(w.obs_offset[l + 1]), int(w.start_frame[l])
        for o in range(o0 + 1, o1):
            yield l, o0, o, fi, fi + (o - o0)


def visual_of(w, st, l, o0, o, fi, fj, obs, **kw):
    return visual(bool(w.estimate_td), obs["TR"], obs["ROW"], obs["s"], obs["pt"][o0], obs["pt"][o], obs["vel"][o0], obs["vel"][o], obs["ctd"][o0],
                  obs["ctd"][o], obs["uvy"][o0], obs["uvy"][o], st.pose[fi], st.pose[fj], st.ex, st.lam[l], st.td, **kw)


def obs_mp(w):
    return dict(TR=mp.mpf(float(w.tr)), ROW=mp.mpf(float(w.row)), s=mp.mpf(float(w.sqrt_info)), pt=to_mp(w.obs_point), vel=to_mp(w.obs_velocity),
                ctd=to_mp(w.obs_cur_td), uvy=to_mp(w.obs_uv_y))


def product_unit(A, uA, B, uB):
    """The unit of A^T B where A, B (absolute values) carry the units uA, uB: first-order propagation uA^T |B| + |A|^T uB — a unit is
    at least the absolute value, so the rounding of the products and of their sum is inside — and the second-order term eps uA^T uB,
    which is all there is where both factors have cancelled to nothing (a landmark seen from two coincident frames)."""
    return uA.T @ B + A.T @ uB + EPS * (uA.T @ uB)


class Statement:
    """The linearization of one window at its state (see the module docstring).  Fields (x: hi, x_lo: the rest, abs_x: the unit):
      cost; g [172]; H [172, 172]; a, b [N]; W [N, 73]                                    the assembled blocks
      vis_H [73, 73], vis_g [73]                                                           the visual terms of the camera part
      imu_H [10, 30, 30], imu_g [10, 30], imu_cost [10], imu_kappa [10]                    per factor over imu_columns(f); zeros if skipped
      prior_A [n, n], prior_b [n], prior_cost, prior_cmap [n]                              J0^T J0, J0^T r, with the column map
    The abs_ fields of the IMU sources are WITHOUT the conditioning factor; units() puts the parts together with it.
    An mpf copy of the assembled blocks is kept in .mp for the certificate."""

    def __init__(self, w, keep_mp=True):
        N = w.N
        st, obs = State(w), obs_mp(w)
        est_ex, est_td = bool(w.estimate_extrinsic), bool(w.estimate_td)
        zero = mp.mpf(0)
        cost = zero
        # ---- visual
        vH = [[zero] * KC for _ in range(KC)]
        vg = [zero] * KC
        a, b, W = [zero] * N, [zero] * N, [[zero] * KC for _ in range(N)]
        abs_vH, abs_vg = np.zeros((KC, KC)), np.zeros(KC)
        abs_a, abs_b, abs_W = np.zeros(N), np.zeros(N), np.zeros((N, KC))
        self.num_factors = 0
        for l, o0, o, fi, fj in observations(w):
            r, J, abs_r, abs_J = visual_of(w, st, l, o0, o, fi, fj, obs)
            if not est_ex:
                J[:, 12:18], abs_J[:, 12:18] = zero, 0.0
            if not est_td:
                J[:, 18], abs_J[:, 18] = zero, 0.0
            rho0, rc, Jc, sq = cauchy(r, J)
            cost += rho0 / 2
            self.num_factors += 1
            cols = list(range(6 * fi, 6 * fi + 6)) + list(range(6 * fj, 6 * fj + 6)) + list(range(66, 73))
            J0, J1 = list(Jc[0, :19]), list(Jc[1, :19])
            l0, l1, r0, r1 = Jc[0, 19], Jc[1, 19], rc[0], rc[1]
            uJ, ur, aJ, ar = float(sq) * abs_J, float(sq) * abs_r, np.abs(to_f(Jc)), np.abs(to_f(rc))
            for p in range(19):  # (fi < fj < ex: cols ascends, so (cols[p], cols[q <= p]) is in the lower triangle)
                cp, x0, x1 = cols[p], J0[p], J1[p]
                if x0 == 0 and x1 == 0:
                    continue
                row = vH[cp]
                for q in range(p + 1):
                    row[cols[q]] += x0 * J0[q] + x1 * J1[q]
                vg[cp] += x0 * r0 + x1 * r1
                W[l][cp] += x0 * l0 + x1 * l1
            a[l] += l0 * l0 + l1 * l1
            b[l] += l0 * r0 + l1 * r1
            ix = np.array(cols)
            abs_vH[np.ix_(ix, ix)] += product_unit(aJ[:, :19], uJ[:, :19], aJ[:, :19], uJ[:, :19])
            abs_vg[ix] += product_unit(aJ[:, :19], uJ[:, :19], ar, ur)
            abs_W[l, ix] += product_unit(aJ[:, :19], uJ[:, :19], aJ[:, 19], uJ[:, 19])
            abs_a[l] += product_unit(aJ[:, 19], uJ[:, 19], aJ[:, 19], uJ[:, 19])
            abs_b[l] += product_unit(aJ[:, 19], uJ[:, 19], ar, ur)
        vHa = np.array(vH, dtype=object).reshape(KC, KC)
        for i in range(KC):
            for j in range(i):
                vHa[j, i] = vHa[i, j]
        # ---- IMU
        G = to_mp(np.asarray(w.g, float))
        iH, ig, ic = _zeros(10, 30, 30), _zeros(10, 30), _zeros(10)
        abs_iH, abs_ig, abs_ic, kap = np.zeros((10, 30, 30)), np.zeros((10, 30)), np.zeros(10), np.ones(10)
        self.imu_kept = np.array([not (w.imu[f].sum_dt > 10.0) for f in range(10)])
        for f in range(10):
            if not self.imu_kept[f]:
                continue
            r, J, abs_r, abs_J, kap[f] = imu(w.imu[f], G, st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1])
            iH[f], ig[f], ic[f] = J.T.dot(J), J.T.dot(r), r.dot(r) / 2
            uJ, ur, aJ, ar = to_f(abs_J), to_f(abs_r), np.abs(to_f(J)), np.abs(to_f(r))
            abs_iH[f], abs_ig[f], abs_ic[f] = product_unit(aJ, uJ, aJ, uJ), product_unit(aJ, uJ, ar, ur), product_unit(ar, ur, ar, ur) / 2
            cost += ic[f]
        # ---- prior
        pr = w.prior if (w.prior is not None and w.prior.valid) else None
        n = pr.n if pr is not None else 0
        pA, pb, pc, cmap = _zeros(n, n), _zeros(n), zero, np.zeros(0, np.int64)
        abs_pA, abs_pb = np.zeros((n, n)), np.zeros(n)
        self.prior_flipped = []
        if pr is not None:
            J0d, r0d = pr.J(), pr.r()
            J0m = to_mp(J0d)
            dx, self.prior_flipped = prior_dx(pr, st)
            rows = [list(J0m[i]) for i in range(n)]
            dxl = list(dx)
            r = _arr([mp.mpf(float(r0d[i])) + mp.fdot(rows[i], dxl) for i in range(n)])
            colsT = [list(J0m[:, j]) for j in range(n)]
            for i in range(n):
                for j in range(i + 1):
                    pA[i, j] = pA[j, i] = mp.fdot(colsT[i], colsT[j])
                pb[i] = mp.fdot(colsT[i], list(r))
            pc = r.dot(r) / 2
            cost += pc
            cmap = prior_columns(pr)
            aJ = np.abs(J0d)
            abs_pA, abs_pb = aJ.T @ aJ, aJ.T @ (np.abs(r0d) + aJ @ np.abs(to_f(dx)))
        # ---- assembled
        act = np.ones(KP, dtype=bool)
        if not est_ex:
            act[66:72] = False
        if not est_td:
            act[72] = False
        H, g = _zeros(KP, KP), _zeros(KP)
        H[:KC, :KC] = vHa
        g[:KC] = _arr(vg)
        for f in range(10):
            ix = np.array(imu_columns(f))
            H[np.ix_(ix, ix)] += iH[f]
            g[ix] += ig[f]
        if n:
            ka = act[cmap]  # (columns of a constant ex / td: the prior's residual keeps their dx, its Jacobian loses them)
            ix = cmap[ka]
            H[np.ix_(ix, ix)] += pA[np.ix_(ka, ka)]
            g[ix] += pb[ka]
        self.active, self.N, self.prior_n, self.prior_cmap = act, N, n, cmap
        Wm = np.array(W, dtype=object).reshape(N, KC)
        self._store(cost=cost, g=g, H=H, a=_arr(a), b=_arr(b), W=Wm, vis_H=vHa, vis_g=_arr(vg), imu_H=iH, imu_g=ig, imu_cost=ic,
                    prior_A=pA, prior_b=pb, prior_cost=pc)
        self.imu_kappa = kap
        self.abs = dict(vis_H=abs_vH, vis_g=abs_vg, imu_H=abs_iH, imu_g=abs_ig, imu_cost=abs_ic, prior_A=abs_pA, prior_b=abs_pb, a=abs_a, b=abs_b, W=abs_W)
        self.mp = dict(cost=cost, g=g, H=H, a=_arr(a), b=_arr(b), W=Wm) if keep_mp else None
        self.span = np.zeros((N, KC), dtype=bool)  # a landmark's span: its track's frames, ex, td
        for l in range(N):
            k = int(w.obs_offset[l + 1] - w.obs_offset[l])
            self.span[l, 6 * int(w.start_frame[l]):6 * (int(w.start_frame[l]) + k)] = True
            self.span[l, 66:73] = True

    def _store(self, **kw):
        self.hi, self.lo = {}, {}
        for k, v in kw.items():
            h, l = split(np.asarray(v, dtype=object))
            self.hi[k], self.lo[k] = h, l

    def diff(self, key, got):
        """|got - statement| entry by entry (a double array; exact to 1e-32 of the statement)."""
        got = np.asarray(got, dtype=np.float64)
        return np.abs((got - self.hi[key]) - self.lo[key])

    def units(self):
        """The sums of absolute terms of the assembled H [172, 172] and g [172]: visual + IMU + prior."""
        aH, ag = np.zeros((KP, KP)), np.zeros(KP)
        aH[:KC, :KC] = self.abs["vis_H"]
        ag[:KC] = self.abs["vis_g"]
        for f in range(10):
            ix = np.array(imu_columns(f))
            aH[np.ix_(ix, ix)] += self.abs["imu_H"][f]
            ag[ix] += self.abs["imu_g"][f]
        if self.prior_n:
            ka = self.active[self.prior_cmap]
            ix = self.prior_cmap[ka]
            aH[np.ix_(ix, ix)] += self.abs["prior_A"][np.ix_(ka, ka)]
            ag[ix] += self.abs["prior_b"][ka]
        return aH, ag


def certificate(w, stm, dps=80):
    """The statement evaluated again at `dps` digits: the largest deviation of any assembled entry, relative to the largest entry of its
    array (the 50-digit result is unchanged at 80 digits to 1e-40, or an intermediate lost more digits than the margin allows)."""
    with mp.workdps(dps):
        hi = Statement(w)
        worst = mp.mpf(0)
        for k in ("cost", "g", "H", "a", "b", "W"):
            x, y = np.asarray(stm.mp[k], dtype=object).ravel(), np.asarray(hi.mp[k], dtype=object).ravel()
            if x.size == 0:
                continue
            scale = max(abs(v) for v in y)
            if scale == 0:
                assert all(v == 0 for v in x), k
                continue
            worst = max(worst, max(abs(p - q) for p, q in zip(x, y)) / scale)
        return float(worst)


# ------------------------------------------------------------------------------------------------------------------------
# the report on one double-precision linearization
# ------------------------------------------------------------------------------------------------------------------------
def _block_metric(d, unit, r0, nr, c0, nc):
    """worst |deviation| of a block in eps x the block's unit; a block without terms must be exactly zero (inf otherwise);
    inside a block, an entry without terms must be exactly zero too."""
    db, ub = d[r0:r0 + nr, c0:c0 + nc], unit[r0:r0 + nr, c0:c0 + nc]
    if np.any(db[ub == 0.0] != 0.0):
        return np.inf
    u = ub.max() if ub.size else 0.0
    if u == 0.0:
        return 0.0
    return float(db.max() / (EPS * u))


def _kind_pair(k1, k2):
    order = {"pose": 0, "sb": 1, "ex": 2, "td": 3}
    a, b = sorted((k1, k2), key=lambda k: order[k])
    if b == "td":
        return "td"
    if b == "ex":
        return "ex"
    return {("pose", "pose"): "pose_pose", ("pose", "sb"): "sb_pose", ("sb", "sb"): "sb_sb"}[(a, b)]


H_METRICS = ("H_pose_pose", "H_sb_pose", "H_sb_sb", "H_ex", "H_td")
G_METRICS = ("g_pose", "g_sb", "g_ex", "g_td")
LM_METRICS = ("a", "b", "W_pose", "W_ex", "W_td")
ASSEMBLED_METRICS = ("cost",) + G_METRICS + H_METRICS + LM_METRICS
VIS_METRICS = ("vis_pose_pose", "vis_ex", "vis_td")
SOURCE_METRICS = VIS_METRICS + ("imu33", "imu_g", "imu_cost", "prior_A")
LINW_METRICS = ("cost",) + G_METRICS + LM_METRICS + SOURCE_METRICS


def report_H(stm, H, rep, worst_block=None):
    aH, _ = stm.units()
    d = stm.diff("H", H)
    for m in H_METRICS:
        rep[m] = 0.0
    for (k1, f1, r0, nr) in BLOCKS:
        for (k2, f2, c0, nc) in BLOCKS:
            m = "H_" + _kind_pair(k1, k2)  # (both triangles of the full matrix: an asymmetric result shows as a deviation)
            v = _block_metric(d, aH, r0, nr, c0, nc)
            if worst_block is not None and v > rep[m]:
                worst_block[m] = (k1, f1, k2, f2)
            rep[m] = max(rep[m], v)


def report_g(stm, g, rep):
    _, ag = stm.units()
    d = stm.diff("g", g)
    for m in G_METRICS:
        rep[m] = 0.0
    for (k, f, r0, nr) in BLOCKS:
        rep["g_" + k] = max(rep["g_" + k], _block_metric(d[:, None], ag[:, None], r0, nr, 0, 1))


def report_landmarks(stm, a, b, W, rep, perm=None):
    """a, b [N], W [N, 73] in the order perm gives (row k of the arrays is landmark perm[k] of the window)."""
    N = stm.N
    for m in LM_METRICS:
        rep[m] = 0.0
    if N == 0:
        return
    perm = np.arange(N) if perm is None else np.asarray(perm)
    for key, got in (("a", a), ("b", b)):
        d = np.abs((np.asarray(got, float) - stm.hi[key][perm]) - stm.lo[key][perm])
        u = stm.abs[key][perm]
        rep[key] = np.inf if np.any(d[u == 0.0] != 0.0) else float((d[u > 0] / (EPS * u[u > 0])).max()) if np.any(u > 0) else 0.0
    d = np.abs((np.asarray(W, float) - stm.hi["W"][perm]) - stm.lo["W"][perm])
    u = stm.abs["W"][perm]
    for (k, f, c0, nc) in CAMERA_BLOCKS:
        m = "W_" + k
        for l in range(N):  # per landmark and per column block
            rep[m] = max(rep[m], _block_metric(d, u, l, 1, c0, nc))


def report(stm, got, perm=None, worst_block=None):
    """got: dict(H [172, 172] full, g, a, b, W, cost).  Every assembled metric."""
    rep = {}
    c = stm.hi["cost"] + stm.lo["cost"]
    rep["cost"] = float(stm.diff("cost", got["cost"]) / (EPS * abs(c))) if c != 0 else (0.0 if got["cost"] == 0 else np.inf)
    report_g(stm, got["g"], rep)
    report_H(stm, got["H"], rep, worst_block)
    report_landmarks(stm, got["a"], got["b"], got["W"], rep, perm)
    return rep


def report_sources(stm, vis, imu_blocks, imu_g, imu_cost, prior_A, rep, lower_only=False):
    """What the strip sweep exposes separately: the visual part of the camera rows [73, 73], per IMU factor its 30 x 30 block (per 3 x 3
    block), gradient [30] and cost, the prior's J0^T J0 [n, n].  lower_only: of an IMU block only the entries whose tangent row is not
    above their tangent column are given (the ones the assembling solve takes)."""
    d = stm.diff("vis_H", vis)
    u = stm.abs["vis_H"]
    for m in VIS_METRICS:
        rep[m] = 0.0
    for (k1, f1, r0, nr) in CAMERA_BLOCKS:
        for (k2, f2, c0, nc) in CAMERA_BLOCKS:
            if c0 > r0:
                continue
            m = "vis_" + _kind_pair(k1, k2)
            rep[m] = max(rep[m], _block_metric(d, u, r0, nr, c0, nc))
    rep["imu33"] = rep["imu_g"] = rep["imu_cost"] = 0.0
    for f in range(10):
        kf = stm.imu_kappa[f] ** IMU_COND_POWER
        d = stm.diff("imu_H", imu_blocks)[f]
        u = kf * stm.abs["imu_H"][f]
        if lower_only:
            cols = np.array(imu_columns(f))
            take = cols[:, None] >= cols[None, :]
            d, u = np.where(take, d, 0.0), np.where(take, u, 0.0)
        if not stm.imu_kept[f]:
            if np.any(np.asarray(imu_blocks)[f] != 0.0):
                rep["imu33"] = np.inf
            continue
        for p in range(0, 30, 3):
            for q in range(0, 30, 3):
                rep["imu33"] = max(rep["imu33"], _block_metric(d, u, p, 3, q, 3))
        dg = stm.diff("imu_g", imu_g)[f]
        ug = stm.abs["imu_g"][f]
        for p in range(0, 30, 3):
            rep["imu_g"] = max(rep["imu_g"], _block_metric(dg[:, None], ug[:, None], p, 3, 0, 1))
        rep["imu_cost"] = max(rep["imu_cost"], float(stm.diff("imu_cost", imu_cost)[f] / (EPS * stm.abs["imu_cost"][f])))
    rep["prior_A"] = 0.0
    if stm.prior_n:
        d, u = stm.diff("prior_A", prior_A), stm.abs["prior_A"]
        rep["prior_A"] = float((d / (EPS * u)).max()) if np.all(u > 0) else np.inf
    return rep


# ------------------------------------------------------------------------------------------------------------------------
# the double-precision comparators
# ------------------------------------------------------------------------------------------------------------------------
def comparator_np(w):
    """tests/np_ref.py: blocks formed from its dense J and r."""
    st = np_ref.St(w)
    cost, r, J = np_ref.assemble(w, st)
    H, g = J.T @ J, J.T @ r
    return dict(H=H[:KP, :KP], g=g[:KP], a=np.diag(H)[KP:].copy(), b=g[KP:].copy(), W=H[KP:, :KC].copy(), cost=cost)


def sources_np(w):
    """The separate sources from np_ref's factors: the window without IMU factors and prior; J^T J, J^T r, cost per factor; J0^T J0."""
    off = []
    from lfvio import abi

    for p in w.imu:
        q = abi.preint_from_array(abi.preint_to_array(p))
        q.sum_dt = 1e9
        off.append(q)
    vis = comparator_np(w.copy(imu=off, prior=None))["H"][:KC, :KC]
    blocks, grads, costs = np.zeros((10, 30, 30)), np.zeros((10, 30)), np.zeros(10)
    st = np_ref.St(w)
    for f in range(10):
        if w.imu[f].sum_dt > 10.0:
            continue
        r, Jpi, Jsi, Jpj, Jsj, _ = np_ref.imu(w.imu[f], w.g, st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1])
        J = np.hstack([Jpi[:, :6], Jsi, Jpj[:, :6], Jsj])
        blocks[f], grads[f], costs[f] = J.T @ J, J.T @ r, 0.5 * r @ r
    A = np.zeros((0, 0))
    if w.prior is not None and w.prior.valid:
        J0 = w.prior.J()
        A = J0.T @ J0
    return vis, blocks, grads, costs, A


def sources_oracle(oracle, w):
    from lfvio import abi

    off = []
    for p in w.imu:
        q = abi.preint_from_array(abi.preint_to_array(p))
        q.sum_dt = 1e9
        off.append(q)
    vis = oracle.linearize(w.copy(imu=off, prior=None))["H"][:KC, :KC]
    blocks, grads, costs = np.zeros((10, 30, 30)), np.zeros((10, 30)), np.zeros(10)
    for f in range(10):
        if w.imu[f].sum_dt > 10.0:
            continue
        r, Jpi, Jsi, Jpj, Jsj, _ = oracle.imu_evaluate(w.imu[f], w.g, w.pose[f], w.speed_bias[f], w.pose[f + 1], w.speed_bias[f + 1])
        J = np.hstack([Jpi[:, :6], Jsi, Jpj[:, :6], Jsj])
        blocks[f], grads[f], costs[f] = J.T @ J, J.T @ r, 0.5 * r @ r
    A = np.zeros((0, 0))
    if w.prior is not None and w.prior.valid:
        J0 = w.prior.J()
        A = J0.T @ J0
    return vis, blocks, grads, costs, A


def full_report(stm, lin, src):
    rep = report(stm, lin)
    report_sources(stm, *src, rep)
    return rep


MARGIN = 16.0
ALL_METRICS = ASSEMBLED_METRICS + SOURCE_METRICS

# Worst figure of each metric over the two comparators (np_ref.assemble, oracle.linearize) per case class of tests/lin_cases.py, as
# tests/test_lin_hp_ref.py prints them (test_comparator_table_reproduces asserts that this table is what they give).  A bar is MARGIN x
# this, with no floor.  Never a device figure.
COMPARATOR_WORST = {
    'regular': {'cost': 14.0, 'g_pose': 1.29, 'g_sb': 0.666, 'g_ex': 0.404, 'g_td': 0.977, 'H_pose_pose': 62.2,
                'H_sb_pose': 7.77, 'H_sb_sb': 4.08, 'H_ex': 3.68, 'H_td': 78.2, 'a': 6.49, 'b': 2.0, 'W_pose': 15.1,
                'W_ex': 2.63, 'W_td': 9.93, 'vis_pose_pose': 62.2, 'vis_ex': 3.68, 'vis_td': 78.2, 'imu33': 0.213,
                'imu_g': 2.05, 'imu_cost': 0.603, 'prior_A': 0.0},
    'prior': {'cost': 49.2, 'g_pose': 0.539, 'g_sb': 0.47, 'g_ex': 0.0725, 'g_td': 0.0595, 'H_pose_pose': 39.1,
              'H_sb_pose': 8.36, 'H_sb_sb': 2.93, 'H_ex': 2.09, 'H_td': 18.1, 'a': 1.63, 'b': 1.02, 'W_pose': 3.56,
              'W_ex': 1.67, 'W_td': 1.31, 'vis_pose_pose': 39.1, 'vis_ex': 2.09, 'vis_td': 18.1, 'imu33': 0.167, 'imu_g': 1.74,
              'imu_cost': 0.343, 'prior_A': 8.04},
    'edge': {'cost': 11.0, 'g_pose': 1.97, 'g_sb': 2.04, 'g_ex': 0.116, 'g_td': 0.194, 'H_pose_pose': 69.0, 'H_sb_pose': 6.96,
             'H_sb_sb': 3.21, 'H_ex': 2.41, 'H_td': 25.9, 'a': 4.23, 'b': 1.06, 'W_pose': 12.3, 'W_ex': 2.04, 'W_td': 7.92,
             'vis_pose_pose': 69.0, 'vis_ex': 2.41, 'vis_td': 25.9, 'imu33': 1.09, 'imu_g': 25.2, 'imu_cost': 1.5,
             'prior_A': 0.0},
    'far': {'cost': 35.5, 'g_pose': 0.00138, 'g_sb': 0.00138, 'g_ex': 7.48e-05, 'g_td': 0.00679, 'H_pose_pose': 0.515,
            'H_sb_pose': 4.63, 'H_sb_sb': 2.94, 'H_ex': 0.000229, 'H_td': 1.76, 'a': 0.477, 'b': 0.0968, 'W_pose': 0.703,
            'W_ex': 0.0025, 'W_td': 0.83, 'vis_pose_pose': 0.937, 'vis_ex': 0.000229, 'vis_td': 1.76, 'imu33': 0.213,
            'imu_g': 0.0745, 'imu_cost': 0.00219, 'prior_A': 0.0},
    'axis': {'cost': 4.8, 'g_pose': 0.412, 'g_sb': 0.525, 'g_ex': 4.16, 'g_td': 41.6, 'H_pose_pose': 50.9, 'H_sb_pose': 6.51,
             'H_sb_sb': 2.88, 'H_ex': 3.15, 'H_td': 219.0, 'a': 17.4, 'b': 275.0, 'W_pose': 131000.0, 'W_ex': 11.2,
             'W_td': 86.9, 'vis_pose_pose': 274.0, 'vis_ex': 3.15, 'vis_td': 219.0, 'imu33': 0.213, 'imu_g': 1.09,
             'imu_cost': 0.302, 'prior_A': 0.0},
    'offs': {'cost': 9.44, 'g_pose': 0.723, 'g_sb': 0.541, 'g_ex': 0.0727, 'g_td': 0.0621, 'H_pose_pose': 60.0,
             'H_sb_pose': 6.49, 'H_sb_sb': 3.34, 'H_ex': 1.02, 'H_td': 13.1, 'a': 2.29, 'b': 2.28, 'W_pose': 12.4,
             'W_ex': 2.11, 'W_td': 2.27, 'vis_pose_pose': 60.0, 'vis_ex': 1.02, 'vis_td': 13.1, 'imu33': 0.206, 'imu_g': 1.69,
             'imu_cost': 0.462, 'prior_A': 0.0},
}


def bar(metric, cls):
    return MARGIN * COMPARATOR_WORST[cls][metric]


def failed_checks(rep, metrics, cls, margin=MARGIN):
    return [(k, rep[k], margin * COMPARATOR_WORST[cls][k]) for k in metrics if not rep[k] <= margin * COMPARATOR_WORST[cls][k]]
