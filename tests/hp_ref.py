"""50-digit restatements (mpmath) of the three feature steps, the reference behind tests/golden/*_hp.npz.

Written from the formulas of lfvio/synth.py (preintegrate), tests/np_ref.py (triangulate, shift_depth) and the comments
of include/lfvio.h.  Every input is a double and is taken exactly; nothing is rounded before the result is returned, and
the results are mpmath numbers (the generator rounds them to double once, at the end).  Quaternions are [w x y z] here;
the packed layout of LfvioPreintegration (delta_q as x y z w) is made by preintegrate_array().

Only the generator (tests/golden/gen_feature_hp.py) and the CPU tests that tie the fixtures to it import this module:
the GPU tests read the files.
"""
import mpmath as mp
import numpy as np

DPS = 50
mp.mp.dps = DPS


def _f(x):
    return mp.mpf(float(x))


def _vec(v):
    return [_f(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[_f(x) for x in row] for row in a])


def to_double(x):
    """Round mpmath scalars / lists / matrices to the nearest double."""
    if isinstance(x, mp.matrix):
        return np.array([[float(x[i, j]) for j in range(x.cols)] for i in range(x.rows)])
    if isinstance(x, (list, tuple)):
        return np.array([float(v) for v in x])
    return float(x)


# ----------------------------------------------------------------------------------------------------------------
# small helpers
# ----------------------------------------------------------------------------------------------------------------
def skew(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx]


def q_to_R(q):
    """The rotation-matrix formula for a unit quaternion, applied as it stands to whatever q is given (the mid-point rule
    feeds it the un-normalised result_delta_q, and so does this restatement)."""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return mp.matrix([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                      [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def q_rot(q, v):
    """v + 2 w (u x v) + 2 u x (u x v), again valid for unit q and used with whatever is given."""
    u = q[1:]
    uv = [2 * c for c in cross(u, v)]
    c2 = cross(u, uv)
    return [v[i] + q[0] * uv[i] + c2[i] for i in range(3)]


def _put(M, r, c, B):
    for i in range(3):
        for j in range(3):
            M[r + i, c + j] = B[i, j]


# ----------------------------------------------------------------------------------------------------------------
# mid-point pre-integration
# ----------------------------------------------------------------------------------------------------------------
def preintegrate(acc0, gyr0, ba, bg, dts, accs, gyrs, noise):
    """Returns dict(sum_dt, delta_p[3], delta_q[4] as w x y z, delta_v[3], jacobian 15x15, covariance 15x15) in mpmath.
    State order p, theta, v, ba, bg; noise = (acc_n, gyr_n, acc_w, gyr_w)."""
    mp.mp.dps = DPS
    an, gn, aw, gw = (_f(x) for x in noise)
    nd = [an * an] * 3 + [gn * gn] * 3 + [an * an] * 3 + [gn * gn] * 3 + [aw * aw] * 3 + [gw * gw] * 3
    I = mp.eye(3)
    J, P = mp.eye(15), mp.zeros(15, 15)
    dp, dv, dq = [mp.mpf(0)] * 3, [mp.mpf(0)] * 3, [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]
    sum_dt = mp.mpf(0)
    a0, g0, ba, bg = _vec(acc0), _vec(gyr0), _vec(ba), _vec(bg)
    dts = np.asarray(dts, dtype=np.float64).reshape(-1)
    accs, gyrs = np.asarray(accs, dtype=np.float64).reshape(-1, 3), np.asarray(gyrs, dtype=np.float64).reshape(-1, 3)
    half, quarter = mp.mpf(1) / 2, mp.mpf(1) / 4
    for k in range(len(dts)):
        dt, a1, g1 = _f(dts[k]), _vec(accs[k]), _vec(gyrs[k])
        a0b, a1b = [a0[i] - ba[i] for i in range(3)], [a1[i] - ba[i] for i in range(3)]
        w = [half * (g0[i] + g1[i]) - bg[i] for i in range(3)]
        un_acc_0 = q_rot(dq, a0b)
        rdq = qmul(dq, [mp.mpf(1), w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2])
        un_acc_1 = q_rot(rdq, a1b)
        un_acc = [half * (un_acc_0[i] + un_acc_1[i]) for i in range(3)]
        rdp = [dp[i] + dv[i] * dt + half * un_acc[i] * dt * dt for i in range(3)]
        rdv = [dv[i] + un_acc[i] * dt for i in range(3)]
        Rw, Ra0, Ra1 = skew(w), skew(a0b), skew(a1b)
        Rdq, Rrdq = q_to_R(dq), q_to_R(rdq)
        ImW = I - Rw * dt
        F = mp.eye(15)
        _put(F, 0, 3, -quarter * (Rdq * Ra0) * dt * dt - quarter * (Rrdq * Ra1 * ImW) * dt * dt)
        _put(F, 0, 6, I * dt)
        _put(F, 0, 9, -quarter * (Rdq + Rrdq) * dt * dt)
        _put(F, 0, 12, quarter * (Rrdq * Ra1) * dt * dt * dt)
        _put(F, 3, 3, ImW)
        _put(F, 3, 12, -I * dt)
        _put(F, 6, 3, -half * (Rdq * Ra0) * dt - half * (Rrdq * Ra1 * ImW) * dt)
        _put(F, 6, 9, -half * (Rdq + Rrdq) * dt)
        _put(F, 6, 12, half * (Rrdq * Ra1) * dt * dt)
        V = mp.zeros(15, 18)
        _put(V, 0, 0, quarter * Rdq * dt * dt)
        _put(V, 0, 3, -quarter * (Rrdq * Ra1) * dt * dt * half * dt)
        _put(V, 0, 6, quarter * Rrdq * dt * dt)
        _put(V, 0, 9, -quarter * (Rrdq * Ra1) * dt * dt * half * dt)
        _put(V, 3, 3, half * I * dt)
        _put(V, 3, 9, half * I * dt)
        _put(V, 6, 0, half * Rdq * dt)
        _put(V, 6, 3, -half * (Rrdq * Ra1) * dt * half * dt)
        _put(V, 6, 6, half * Rrdq * dt)
        _put(V, 6, 9, -half * (Rrdq * Ra1) * dt * half * dt)
        _put(V, 9, 12, I * dt)
        _put(V, 12, 15, I * dt)
        VN = V.copy()
        for j in range(18):
            for i in range(15):
                VN[i, j] = V[i, j] * nd[j]
        J = F * J
        P = F * P * F.T + VN * V.T
        dp, dv = rdp, rdv
        nrm = mp.sqrt(sum(c * c for c in rdq))
        dq = [c / nrm for c in rdq]
        sum_dt += dt
        a0, g0 = a1, g1
    return dict(sum_dt=sum_dt, delta_p=dp, delta_q=dq, delta_v=dv, jacobian=J, covariance=P)


def preintegrate_array(res, ba, bg):
    """The 467 doubles of abi.preint_to_array: sum_dt, delta_p, delta_q (x y z w), delta_v, ba, bg, jacobian, covariance."""
    q = res["delta_q"]
    return np.concatenate([[float(res["sum_dt"])], to_double(res["delta_p"]), to_double([q[1], q[2], q[3], q[0]]),
                           to_double(res["delta_v"]), np.asarray(ba, float), np.asarray(bg, float),
                           to_double(res["jacobian"]).reshape(-1), to_double(res["covariance"]).reshape(-1)])


# ----------------------------------------------------------------------------------------------------------------
# triangulation
# ----------------------------------------------------------------------------------------------------------------
def triangulate_one(start, pts, Ps, Rs, tic, ric):
    """One landmark first seen in frame `start` with observation points pts[k, 3] in frames start .. start + k - 1.
    Returns (d, sigma[4], scale): d the signed depth X . pts[0] of the null vector of the 2k x 4 system (before the
    `d < 0 -> init_depth` branch), the singular values in descending order, and |X| |pts[0]| (what d cancels from)."""
    mp.mp.dps = DPS
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    tic, ric = mp.matrix(_vec(tic)), _mat(ric)
    i = int(start)
    Ri = _mat(Rs[i])
    t0, R0 = mp.matrix(_vec(Ps[i])) + Ri * tic, Ri * ric
    rows = []
    for o in range(len(pts)):
        Rj = _mat(Rs[i + o])
        t1, R1 = mp.matrix(_vec(Ps[i + o])) + Rj * tic, Rj * ric
        t, R = R0.T * (t1 - t0), R0.T * R1
        Rt = R.T
        mt = -(Rt * t)
        Pm = [[Rt[r, 0], Rt[r, 1], Rt[r, 2], mt[r]] for r in range(3)]
        p = _vec(pts[o])
        n = mp.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        f = [c / n for c in p]
        rows.append([f[0] * Pm[2][c] - f[2] * Pm[0][c] for c in range(4)])
        rows.append([f[1] * Pm[2][c] - f[2] * Pm[1][c] for c in range(4)])
    U, S, Vt = mp.svd_r(mp.matrix(rows), full_matrices=False, compute_uv=True)
    sig = sorted((S[c] for c in range(4)), reverse=True)
    c4 = min(range(4), key=lambda c: S[c])
    v = [Vt[c4, c] for c in range(4)]
    X = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
    p0 = _vec(pts[0])
    d = X[0] * p0[0] + X[1] * p0[1] + X[2] * p0[2]
    scale = mp.sqrt(sum(c * c for c in X)) * mp.sqrt(sum(c * c for c in p0))
    return d, sig, scale


def triangulate(start_frame, obs_offset, obs_point, Ps, Rs, tic, ric, depth, init_depth):
    """All landmarks of one call.  Returns (depth_out, d_raw, sigma[N, 4], scale[N]) as doubles; landmarks that come in
    with a positive depth keep it (d_raw, sigma and scale are still those of their system)."""
    N = len(start_frame)
    obs_point = np.asarray(obs_point, dtype=np.float64).reshape(-1, 3)
    out, raw, sig, scale = np.array(depth, dtype=np.float64), np.zeros(N), np.zeros((N, 4)), np.zeros(N)
    for l in range(N):
        d, s, sc = triangulate_one(start_frame[l], obs_point[obs_offset[l]:obs_offset[l + 1]], Ps, Rs, tic, ric)
        raw[l], sig[l], scale[l] = float(d), to_double(s), float(sc)
        if not out[l] > 0:
            out[l] = float(d) if d >= 0 else float(init_depth)
    return out, raw, sig, scale


# ----------------------------------------------------------------------------------------------------------------
# removeBackShiftDepth's arithmetic
# ----------------------------------------------------------------------------------------------------------------
def shift_depth(uv_i, marg_R, marg_P, new_R, new_P, init_depth, depth):
    """|new_R^T (marg_R (uv depth) + marg_P - new_P)| per landmark, init_depth where that is 0.  Returns doubles."""
    mp.mp.dps = DPS
    uv = np.asarray(uv_i, dtype=np.float64).reshape(-1, 3)
    mR, nRT = _mat(np.reshape(marg_R, (3, 3))), _mat(np.reshape(new_R, (3, 3))).T
    mP, nP = mp.matrix(_vec(marg_P)), mp.matrix(_vec(new_P))
    out = np.zeros(len(uv))
    for l in range(len(uv)):
        d = _f(depth[l])
        pj = nRT * (mR * mp.matrix([_f(c) * d for c in uv[l]]) + mP - nP)
        r = mp.sqrt(pj[0] * pj[0] + pj[1] * pj[1] + pj[2] * pj[2])
        out[l] = float(r) if r > 0 else float(init_depth)
    return out
