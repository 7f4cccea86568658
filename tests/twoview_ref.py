"""Restatements of the online camera-IMU rotation calibration (initial/initial_ex_rotation.cpp), the reference behind
tests/test_two_view.py and tests/test_exrot_host.py.

Two of them, written from the line references of include/lfvio.h and of the comments below, not from the source text:

  numpy, double precision    two_view(): compute_E_21 (:69-100), check_inliers (:101-155, FLOAT threshold, FLOAT score
                             taking double terms in match order), the selection (:197-202), the refit (:204-218),
                             decomposeE (:321-336) with the det R1 = -1 retry of :271-275, testTriangulation (:289-319,
                             :338-353) and the choice of :276-284; ExRotCalib: CalibrationExRotation (:13-67)
  mpmath, 50 digits          hp_*: the same steps with every input taken exactly and nothing rounded before the end (the
                             score: residuals and terms in 50 digits, the accumulator rounded to float after every
                             term, because the float accumulator is part of what is restated); used by tests/golden/gen_twoview_hp.py only

Singular vectors: the 50-digit side takes them from the symmetric eigenproblem of A^T A — at 60 digits the squared
condition number (< 1e12 for every fixture) leaves 48 good ones.
"""
import numpy as np

THR32 = np.float32(0.00872653549837)
THR = float(THR32)
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


# ----------------------------------------------------------------------------------------------------------------
# numpy
# ----------------------------------------------------------------------------------------------------------------
def system(bl, br):
    """Rows [b_r.x b_l, b_r.y b_l, b_r.z b_l] (:76-81)."""
    bl, br = np.asarray(bl, np.float64), np.asarray(br, np.float64)
    return np.hstack([br[:, 0:1] * bl, br[:, 1:2] * bl, br[:, 2:3] * bl])


def compute_E(bl, br, info=None):
    A = system(bl, br)
    _, s, Vt = np.linalg.svd(A, full_matrices=True)
    E0 = Vt[8].reshape(3, 3)
    U, lam, Vt3 = np.linalg.svd(E0)
    if info is not None:
        info["cond_A"] = s[0] / s[7]
        info["gap_E0"] = lam[0] / (lam[1] - lam[2])
        info["rank2"] = lam[0] / lam[1]
    lam = lam.copy()
    lam[2] = 0.0
    return U @ np.diag(lam) @ Vt3


def residuals(E, bl, br):
    """(r2, r1): |(E b_l) . b_r| / |E b_l| and |(E^T b_r) . b_l| / |E^T b_r|; E [..., 3, 3]."""
    with np.errstate(all="ignore"):
        e2 = np.einsum("...ij,nj->...ni", E, bl)
        r2 = np.abs(np.einsum("...ni,ni->...n", e2, br) / np.sqrt(np.einsum("...ni,...ni->...n", e2, e2)))
        e1 = np.einsum("...ji,nj->...ni", E, br)
        r1 = np.abs(np.einsum("...ni,ni->...n", e1, bl) / np.sqrt(np.einsum("...ni,...ni->...n", e1, e1)))
    return r2, r1


def check_inliers(E, bl, br, margin=None):
    """E [S, 3, 3] or [3, 3] -> (float32 score(s), uint8 mask(s)).  margin (a one-element list): the smallest
    |residual - thr| / thr met on the way (condition C2)."""
    E = np.asarray(E, np.float64)
    single = E.ndim == 2
    Es = E[None] if single else E
    score = np.zeros(len(Es), np.float32)
    mask = np.zeros((len(Es), len(bl)), np.uint8)
    for s0 in range(0, len(Es), 64):
        r2, r1 = residuals(Es[s0:s0 + 64], bl, br)
        with np.errstate(all="ignore"):
            p2, p1 = ~(THR < r2), ~(THR < r1)
            c2, c1 = (THR - r2) ** 2, (THR - r1) ** 2
        sc = np.zeros(len(r2), np.float32)
        with np.errstate(all="ignore"):
            for i in range(len(bl)):
                a = (sc.astype(np.float64) + c2[:, i]).astype(np.float32)
                sc = np.where(p2[:, i], a, sc)
                b = (sc.astype(np.float64) + c1[:, i]).astype(np.float32)
                sc = np.where(p2[:, i] & p1[:, i], b, sc)
        score[s0:s0 + 64] = sc
        mask[s0:s0 + 64] = p2 & p1
        if margin is not None:
            m = np.abs(r2 - THR) / THR
            m1 = np.where(p2, np.abs(r1 - THR) / THR, np.inf)
            margin[0] = min(margin[0], float(np.nanmin(m)), float(np.nanmin(m1)))
    return (score[0], mask[0]) if single else (score, mask)


def decompose(E):
    """decomposeE with the retry of :271-275 -> R1, R2, t (the candidates are (R1 | R2, +-t))."""
    U, _, Vt = np.linalg.svd(E)
    R1, R2 = U @ W @ Vt, U @ W.T @ Vt
    if np.linalg.det(R1) + 1.0 < 1e-9:
        U, _, Vt = np.linalg.svd(-E)
        R1, R2 = U @ W @ Vt, U @ W.T @ Vt
    return R1, R2, U[:, 2].copy()


def design(bl, br, R, t):
    """The 4 x 4 systems of triangulatePoint (:341-346) for Pose0 = [I | 0], Pose1 = [R | t]; [N, 4, 4]."""
    P1 = np.hstack([R, t.reshape(3, 1)])
    D = np.zeros((len(bl), 4, 4))
    D[:, 0, 0], D[:, 0, 2] = -bl[:, 2], bl[:, 0]
    D[:, 1, 1], D[:, 1, 2] = -bl[:, 2], bl[:, 1]
    D[:, 2] = br[:, 0:1] * P1[2] - br[:, 2:3] * P1[0]
    D[:, 3] = br[:, 1:2] * P1[2] - br[:, 2:3] * P1[1]
    return D


def front_count(bl, br, R, t):
    Vt = np.linalg.svd(design(bl, br, R, t))[2]
    with np.errstate(all="ignore"):
        X = Vt[:, 3, :3] / Vt[:, 3, 3:4]
        dl = np.einsum("ni,ni->n", bl, X)
        dr = np.einsum("ni,ni->n", br, X @ R.T + t)
        return int(np.count_nonzero((dl > 0) & (dr > 0)))


def two_view(bl, br, samples, all_hypotheses=False):
    """dict with the fields of LfvioTwoViewOut (+ mask, E_all, score_all, the condition numbers of the metrics' units and
    the facts behind conditions C1 - C3)."""
    bl, br = np.ascontiguousarray(bl, np.float64), np.ascontiguousarray(br, np.float64)
    samples = np.asarray(samples, np.int32).reshape(-1, 8)
    N, S = len(bl), len(samples)
    E_all = np.zeros((S, 3, 3))
    cond = np.zeros((S, 2))
    for k, idx in enumerate(samples):
        info = {}
        E_all[k] = compute_E(bl[idx], br[idx], info)
        cond[k] = info["cond_A"], info["gap_E0"]
    score_all, mask_all = check_inliers(E_all, bl, br)
    out = dict(E_all=E_all.reshape(S, 9), score_all=score_all, cond_all=cond, status=1, best_sample=-1, num_inliers=0, best_score=0.0)
    best, bs = -1, 0.0
    for k in range(S):
        if bs < float(score_all[k]):
            bs, best = float(score_all[k]), k
    if best < 0:
        return out
    out.update(best_sample=best, best_score=bs, num_inliers=int(mask_all[best].sum()))
    # C1: the runner-up among sample sets that differ from the winner's
    other = [float(score_all[k]) for k in range(S) if not np.array_equal(np.sort(samples[k]), np.sort(samples[best]))]
    out["c1_gap"] = (bs - max(other)) / bs if other and max(other) > 0 else np.inf
    margin = [np.inf]
    check_inliers(E_all[best], bl, br, margin)
    if out["num_inliers"] < 8:
        return out
    sel = mask_all[best].astype(bool)
    info = {}
    E = compute_E(bl[sel], br[sel], info)
    _, mask = check_inliers(E, bl, br, margin)
    R1, R2, t = decompose(E)
    fr = np.array([front_count(bl, br, R1, t), front_count(bl, br, R1, -t), front_count(bl, br, R2, t), front_count(bl, br, R2, -t)]) / float(N)
    ratio1, ratio2 = max(fr[0], fr[1]), max(fr[2], fr[3])
    out.update(status=0, num_inliers=int(mask.sum()), mask=mask, E=E.reshape(9), R_cand=np.stack([R1, R2]), t_cand=t, front=fr,
               R_rel=(R1 if ratio1 > ratio2 else R2).T.copy(), cond_refit=(info["cond_A"], info["gap_E0"]), rank2=info["rank2"],
               c2_margin=margin[0], c3_gap=abs(ratio1 - ratio2) * N, pre_inliers=int(sel.sum()))
    return out


def e_distance(a, b):
    """Frobenius distance of two 3 x 3 matrices after normalisation, up to sign."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def rot_angle(Ra, Rb):
    """Angle of Ra^T Rb [rad], accurate near zero (from the skew part and the trace)."""
    D = np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


def candidate_distance(got_R, got_t, got_front, ref_R, ref_t, ref_front):
    """The four candidates (R1 | R2, +-t) as a SET: the device and a restatement may name them differently (which rotation is
    R1 and the sign of t follow the signs an SVD happens to give its vectors).  Returns (worst angle over the matched
    candidates [rad], the device's front[] reordered to the reference's naming)."""
    got_R, ref_R = np.asarray(got_R).reshape(2, 3, 3), np.asarray(ref_R).reshape(2, 3, 3)
    got_t, ref_t = np.asarray(got_t).reshape(3), np.asarray(ref_t).reshape(3)
    swap = rot_angle(got_R[0], ref_R[0]) + rot_angle(got_R[1], ref_R[1]) > rot_angle(got_R[0], ref_R[1]) + rot_angle(got_R[1], ref_R[0])
    flip = float(got_t @ ref_t) < 0
    ang = max(rot_angle(got_R[1 if swap else 0], ref_R[0]), rot_angle(got_R[0 if swap else 1], ref_R[1]))
    ct = float(np.clip(abs(got_t @ ref_t) / (np.linalg.norm(got_t) * np.linalg.norm(ref_t)), 0, 1))
    st = np.linalg.norm(np.cross(got_t, ref_t)) / (np.linalg.norm(got_t) * np.linalg.norm(ref_t))
    ang = max(ang, float(np.arctan2(st, ct)))
    order = [(2 * (r ^ swap)) + (s ^ flip) for r in (0, 1) for s in (0, 1)]
    return ang, np.asarray(got_front)[order]


# ----------------------------------------------------------------------------------------------------------------
# CalibrationExRotation (:13-67)
# ----------------------------------------------------------------------------------------------------------------
def mat_to_quat(R):
    """Quaternion [w x y z] of a rotation matrix by the branch on the trace and the largest diagonal entry."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def quat_to_mat(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def angular_distance(a, b):
    d = quat_mul(a, np.array([b[0], -b[1], -b[2], -b[3]]))
    return 2.0 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0]))


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


class ExRotCalib:
    """InitialEXRotation's state and CalibrationExRotation."""

    def __init__(self, window_size=10):
        self.window_size = window_size
        self.frame_count = 0
        self.Rc, self.Rimu, self.Rc_g = [np.eye(3)], [np.eye(3)], [np.eye(3)]
        self.ric = np.eye(3)
        self.sv = np.zeros(4)

    def stack(self):
        A = np.zeros((4 * self.frame_count, 4))
        for i in range(1, self.frame_count + 1):
            r1, r2 = mat_to_quat(self.Rc[i]), mat_to_quat(self.Rc_g[i])
            ang = 180.0 / np.pi * angular_distance(r1, r2)
            huber = 5.0 / ang if ang > 5.0 else 1.0
            L, R = np.zeros((4, 4)), np.zeros((4, 4))
            w, q = r1[0], r1[1:]
            L[:3, :3], L[:3, 3], L[3, :3], L[3, 3] = w * np.eye(3) + skew(q), q, -q, w
            rq = mat_to_quat(self.Rimu[i])
            w, q = rq[0], rq[1:]
            R[:3, :3], R[:3, 3], R[3, :3], R[3, 3] = w * np.eye(3) - skew(q), q, -q, w
            A[4 * (i - 1):4 * i] = huber * (L - R)
        return A

    def push(self, Rc, delta_q_wxyz=None, Rimu=None):
        """-> (success, ric, singular values).  The IMU rotation as the quaternion delta_q or as its matrix."""
        self.frame_count += 1
        Rq = quat_to_mat(np.asarray(delta_q_wxyz, np.float64)) if Rimu is None else np.asarray(Rimu, np.float64).reshape(3, 3).copy()
        self.Rc.append(np.asarray(Rc, np.float64).reshape(3, 3).copy())
        self.Rimu.append(Rq)
        self.Rc_g.append(np.linalg.inv(self.ric) @ Rq @ self.ric)
        A = self.stack()
        _, s, Vt = np.linalg.svd(A, full_matrices=True)
        x = Vt[3]  # (x, y, z, w)
        self.ric = np.linalg.inv(quat_to_mat(np.array([x[3], x[0], x[1], x[2]])))
        self.sv = s
        return bool(self.frame_count >= self.window_size and s[2] > 0.25), self.ric.copy(), s.copy()


# ----------------------------------------------------------------------------------------------------------------
# mpmath, 50 digits (the generator's side)
# ----------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath as mp
    mp.mp.dps = 60
    return mp


def _mpm(a):
    mp = _mp()
    a = np.asarray(a, np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a])


def _eig_sorted(G):
    """Eigenvalues ascending and the eigenvector columns of a symmetric mp.matrix."""
    mp = _mp()
    ev, Q = mp.eigsy(G)
    order = sorted(range(len(ev)), key=lambda i: ev[i])
    return [ev[i] for i in order], [[Q[r, i] for r in range(Q.rows)] for i in order]


def hp_compute_E(bl, br):
    """-> (E as an mp.matrix, sigma_1/sigma_8 of the system, sigma_1/(sigma_2 - sigma_3) and sigma_1/sigma_2 of E_0, V, sigma of E_0)."""
    mp = _mp()
    A = _mpm(system(bl, br))
    ev, vec = _eig_sorted(A.T * A)
    v = vec[0]
    E0 = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            E0[i, j] = v[3 * i + j]
    ev3, vec3 = _eig_sorted(E0.T * E0)
    sg = [mp.sqrt(max(e, mp.mpf(0))) for e in ev3]  # ascending: sigma_3, sigma_2, sigma_1
    v3 = mp.matrix(vec3[0])
    E = E0 - (E0 * v3) * v3.T
    return E, mp.sqrt(ev[8] / ev[1]), sg[2] / (sg[1] - sg[0]), sg[2] / sg[1], E0


def hp_residuals(E, bl, br):
    """Per match (r2, r1) as mpmath numbers."""
    mp = _mp()
    out = []
    for l, r in zip(np.asarray(bl, np.float64), np.asarray(br, np.float64)):
        l, r = mp.matrix([mp.mpf(float(x)) for x in l]), mp.matrix([mp.mpf(float(x)) for x in r])
        e2, e1 = E * l, E.T * r
        r2 = abs((e2.T * r)[0] / mp.sqrt((e2.T * e2)[0]))
        r1 = abs((e1.T * l)[0] / mp.sqrt((e1.T * e1)[0]))
        out.append((r2, r1))
    return out


def hp_check_inliers(E, bl, br):
    """-> (float32 score, mask, smallest |residual - thr| / thr met)."""
    mp = _mp()
    thr = mp.mpf(THR)
    score, mask, margin = np.float32(0.0), np.zeros(len(bl), np.uint8), mp.inf
    for i, (r2, r1) in enumerate(hp_residuals(E, bl, br)):
        margin = min(margin, abs(r2 - thr) / thr)
        if thr < r2:
            continue
        score = np.float32(float(mp.mpf(float(score)) + (thr - r2) ** 2))
        margin = min(margin, abs(r1 - thr) / thr)
        if thr < r1:
            continue
        score = np.float32(float(mp.mpf(float(score)) + (thr - r1) ** 2))
        mask[i] = 1
    return score, mask, float(margin)


def hp_decompose(E):
    """R1 = U W V^T, R2 = U W^T V^T, t = u_3 with u_3 = u_1 x u_2, v_3 = v_1 x v_2 (proper rotations)."""
    mp = _mp()
    ev, vec = _eig_sorted(E.T * E)
    v1, v2 = mp.matrix(vec[2]), mp.matrix(vec[1])
    u1, u2 = E * v1 / mp.sqrt(ev[2]), E * v2 / mp.sqrt(ev[1])

    def cross(a, b):
        return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    u3, v3 = cross(u1, u2), cross(v1, v2)
    a = u2 * v1.T - u1 * v2.T
    b = u3 * v3.T
    return a + b, b - a, u3


def hp_front_count(bl, br, R, t):
    mp = _mp()
    Rn = np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])
    tn = np.array([float(t[i]) for i in range(3)])
    D = design(np.asarray(bl, np.float64), np.asarray(br, np.float64), Rn, tn)  # layout only; rebuilt exactly below
    P1 = mp.matrix(3, 4)
    for i in range(3):
        for j in range(3):
            P1[i, j] = R[i, j]
        P1[i, 3] = t[i]
    n = 0
    for k in range(len(D)):
        l = [mp.mpf(float(x)) for x in bl[k]]
        r = [mp.mpf(float(x)) for x in br[k]]
        M = mp.matrix(4, 4)
        M[0, 0], M[0, 2], M[1, 1], M[1, 2] = -l[2], l[0], -l[2], l[1]
        for c in range(4):
            M[2, c] = r[0] * P1[2, c] - r[2] * P1[0, c]
            M[3, c] = r[1] * P1[2, c] - r[2] * P1[1, c]
        _, vec = _eig_sorted(M.T * M)
        q = vec[0]
        if q[3] == 0:
            continue
        X = [q[0] / q[3], q[1] / q[3], q[2] / q[3]]
        Xr = [sum(R[i, j] * X[j] for j in range(3)) + t[i] for i in range(3)]
        if sum(l[i] * X[i] for i in range(3)) > 0 and sum(r[i] * Xr[i] for i in range(3)) > 0:
            n += 1
    return n


def hp_to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
