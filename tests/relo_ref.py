"""Independent float64 numpy statement of the relocalization branch of optimization() (test infrastructure).

Built from tests/np_ref.py: the relo factor is np_ref.visual(use_td=False, ...) — the plain ProjectionFactor with
pts_j = (x, y, 1) (estimator.cpp:777-808, factor/projection_factor.cpp) — on (para_Pose[start], relo_Pose, para_Ex_Pose,
para_Feature[l]); `assemble` gains the relo block (6 local columns behind the landmarks) and `solve` is np_ref.solve's
Ceres 1.12 dogleg loop over the augmented state, with the trace fields the device reports (gradient max-norm
max |x - Plus(x, -g)| at every new point, include/lfvio.h).  `relo_tail` states the relo tail of double2vector()
(estimator.cpp:603-625).
"""
from math import atan2, cos, pi, sin

import numpy as np

import np_ref
from np_ref import KP, OFF_EX, OFF_TD, St, off_pose, off_sb


class Relo:
    def __init__(self, frame, relo_pose, landmark=(), match_point=()):
        self.frame = int(frame)
        self.relo_pose = np.array(relo_pose, dtype=float)
        self.landmark = np.array(landmark, dtype=int).reshape(-1)
        self.match_point = np.array(match_point, dtype=float).reshape(-1, 2)

    @property
    def K(self):
        return int(self.landmark.size)


def relo_factor(w, st, l, relo_pose, xy):
    """r(2), J_pose_start(2x6), J_relo(2x6), J_ex(2x6), J_lam(2) — ProjectionFactor(pts_i = first observation, (x, y, 1))."""
    o0 = int(w.obs_offset[l])
    fi = int(w.start_frame[l])
    z3 = np.zeros(3)
    pts_j = np.array([xy[0], xy[1], 1.0])
    r, Ji, Jj, Jex, Jl, _ = np_ref.visual(False, w.tr, w.row, w.sqrt_info, w.obs_point[o0], pts_j, z3, z3, 0.0, 0.0, 0.0, 0.0,
                                          st.pose[fi], relo_pose, st.ex, st.lam[l], st.td)
    return r, Ji[:, :6], Jj[:, :6], Jex[:, :6], Jl


def assemble(w, st, relo, relo_pose, want_J=True):
    """np_ref.assemble plus the relo factors; columns [0, KP) pose side, [KP, KP + N) landmarks, [KP + N, KP + N + 6) relo."""
    cost, r, J = np_ref.assemble(w, st, want_J)
    N = w.N
    rows_r = [r]
    rows_J = [np.hstack([J, np.zeros((J.shape[0], 6))])] if want_J else None
    for k in range(relo.K):
        l = int(relo.landmark[k])
        rr, Ji, Jr, Jex, Jl = relo_factor(w, st, l, relo_pose, relo.match_point[k])
        Jloc = np.zeros((2, 19))
        Jloc[:, 0:6], Jloc[:, 6:12] = Ji, Jr
        if w.estimate_extrinsic:
            Jloc[:, 12:18] = Jex
        Jloc[:, 18] = Jl
        rho0, rc, Jc = np_ref.cauchy_correct(rr, Jloc)
        cost += 0.5 * rho0
        rows_r.append(rc)
        if want_J:
            Jrow = np.zeros((2, KP + N + 6))
            fi = int(w.start_frame[l])
            Jrow[:, off_pose(fi):off_pose(fi) + 6] += Jc[:, 0:6]
            Jrow[:, KP + N:KP + N + 6] += Jc[:, 6:12]
            Jrow[:, OFF_EX:OFF_EX + 6] += Jc[:, 12:18]
            Jrow[:, KP + l] += Jc[:, 18]
            rows_J.append(Jrow)
    return cost, np.concatenate(rows_r), (np.vstack(rows_J) if want_J else None)


def active_mask(w, relo):
    return np.concatenate([np_ref.active_mask(w), np.full(6, relo.K > 0)])


def xvec(w, st, relo_pose, relo):
    v = st.vec(w)
    return np.concatenate([v, relo_pose]) if relo.K > 0 else v


def grad_max_norm(w, st, relo_pose, relo, g):
    """Ceres' gradient_max_norm = max |x - Plus(x, -g)| over the active blocks (g: unscaled J^T r over all columns)."""
    N = w.N
    m = 0.0

    def pose_part(x, gb):
        return np.abs(x - np_ref.pose_plus(x, -gb)).max()

    for f in range(11):
        m = max(m, pose_part(st.pose[f], g[off_pose(f):off_pose(f) + 6]), np.abs(g[off_sb(f):off_sb(f) + 9]).max())
    if w.estimate_extrinsic:
        m = max(m, pose_part(st.ex, g[OFF_EX:OFF_EX + 6]))
    if w.estimate_td:
        m = max(m, abs(g[OFF_TD]))
    if relo.K > 0:
        m = max(m, pose_part(relo_pose, g[KP + N:KP + N + 6]))
    if N:
        m = max(m, np.abs(g[KP:KP + N]).max())
    return m


def solve(w, relo, radius=1e4, function_tolerance=1e-6, cases=None):
    """Ceres 1.12 TrustRegionMinimizer + TRADITIONAL_DOGLEG over the augmented state (np_ref.solve, literal).

    cases: optional list; every dogleg step appends its case: 0 Gauss-Newton, 1 Cauchy point, 2 interpolation with the
    beta = (d - c) / |b - a|^2 form (c <= 0), 3 interpolation with the beta = (r^2 - |a|^2) / (d + c) form (c > 0)."""
    act = active_mask(w, relo)
    N = w.N
    x = St(w)
    xr = relo.relo_pose.copy()
    mu = 1e-8
    reuse = False
    dogleg_step_norm = 0.0
    cost, r, Jfull = assemble(w, x, relo, xr)
    gm = grad_max_norm(w, x, xr, relo, Jfull.T @ r)
    J = Jfull[:, act]
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(axis=0)))
    J = J * scale
    x_norm = np.linalg.norm(xvec(w, x, xr, relo))
    trace = [dict(cost=cost, cost_change=0.0, gradient_max_norm=gm, step_norm=0.0, relative_decrease=0.0, radius=radius,
                  valid=0, successful=0)]
    iteration, invalid, term = 0, 0, 1
    if gm <= 1e-10:
        return x, xr, trace, 0
    while True:
        if iteration >= w.max_num_iterations:
            term = 1
            break
        if radius <= 1e-32:
            term = 0
            break
        iteration += 1
        failure = False
        if not reuse:
            reuse = True
            diag = np.sqrt(np.clip((J * J).sum(axis=0), 1e-6, 1e32))
            grad = (J.T @ r) / diag
            Jg = J @ (grad / diag)
            alpha = (grad @ grad) / (Jg @ Jg)
            ok = False
            while mu < 1.0:
                lm = diag * np.sqrt(mu)
                A = J.T @ J + np.diag(lm * lm)
                try:
                    L = np.linalg.cholesky(A)
                    y = np.linalg.solve(L.T, np.linalg.solve(L, J.T @ r))
                    if np.all(np.isfinite(y)):
                        ok = True
                        break
                except np.linalg.LinAlgError:
                    pass
                mu *= 10.0
            if ok:
                gn = -diag * y
            else:
                failure = True
        valid = False
        if not failure:
            gnorm, gnn = np.linalg.norm(grad), np.linalg.norm(gn)
            if gnn <= radius:
                step, dogleg_step_norm = gn.copy(), gnn
                case = 0
            elif gnorm * alpha >= radius:
                step, dogleg_step_norm = -(radius / gnorm) * grad, radius
                case = 1
            else:
                b_dot_a = -alpha * (grad @ gn)
                a2 = (alpha * gnorm) ** 2
                bma2 = a2 - 2 * b_dot_a + gnn ** 2
                c = b_dot_a - a2
                d = np.sqrt(c * c + bma2 * (radius ** 2 - a2))
                beta = (d - c) / bma2 if c <= 0 else (radius * radius - a2) / (d + c)
                case = 2 if c <= 0 else 3
                step = (-alpha * (1 - beta)) * grad + beta * gn
                dogleg_step_norm = np.linalg.norm(step)
            if cases is not None:
                cases.append(case)
            step = step / diag
            mr = J @ step
            model_cost_change = -mr @ (r + mr / 2.0)
            valid = model_cost_change > 0
        if not valid:
            invalid += 1
            if invalid >= 5:
                term = 2
                break
            mu *= 10.0
            reuse = False
            trace.append(dict(cost=cost, cost_change=0.0, gradient_max_norm=0.0, step_norm=0.0, relative_decrease=0.0,
                              radius=radius, valid=0, successful=0))
            continue
        invalid = 0
        delta = np.zeros(KP + N + 6)
        delta[act] = step * scale
        cand = np_ref.plus(w, x, delta[:KP + N])
        cand_r = np_ref.pose_plus(xr, delta[KP + N:]) if relo.K > 0 else xr.copy()
        cand_cost, _, _ = assemble(w, cand, relo, cand_r, want_J=False)
        step_norm = np.linalg.norm(xvec(w, x, xr, relo) - xvec(w, cand, cand_r, relo))
        if step_norm <= 1e-8 * (x_norm + 1e-8):
            term = 0
            break
        cost_change = cost - cand_cost
        if abs(cost_change) <= function_tolerance * cost:
            term = 0
            break
        rd = cost_change / model_cost_change
        if rd > 1e-3:
            x, xr = cand, cand_r
            x_norm = np.linalg.norm(xvec(w, x, xr, relo))
            cost, r, Jfull = assemble(w, x, relo, xr)
            J = Jfull[:, act] * scale
            if rd < 0.25:
                radius *= 0.5
            if rd > 0.75:
                radius = max(radius, 3.0 * dogleg_step_norm)
            mu = max(1e-8, 2.0 * mu / 10.0)
            reuse = False
            trace.append(dict(cost=cost, cost_change=cost_change, gradient_max_norm=np.nan, step_norm=step_norm,
                              relative_decrease=rd, radius=radius, valid=1, successful=1))
            done_now = iteration >= w.max_num_iterations or radius <= 1e-32
            if not done_now:
                gm = grad_max_norm(w, x, xr, relo, Jfull.T @ r)
                trace[-1]["gradient_max_norm"] = gm
                if gm <= 1e-10:
                    term = 0
                    break
        else:
            radius *= 0.5
            reuse = True
            trace.append(dict(cost=cand_cost, cost_change=cost_change, gradient_max_norm=0.0, step_norm=step_norm,
                              relative_decrease=rd, radius=radius, valid=1, successful=0))
    return x, xr, trace, term


def objective_gradient(w, st, relo, relo_pose):
    """Unscaled J^T r of the full objective (relo factors included) over the active columns."""
    _, r, J = assemble(w, st, relo, relo_pose)
    return (J.T @ r)[active_mask(w, relo)]


# ---------------------------------------------------------------------------------------------------------------
# double2vector()'s relo tail (estimator.cpp:603-625)
# ---------------------------------------------------------------------------------------------------------------
def R2ypr(R):
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = atan2(n[1], n[0])
    p = atan2(-n[2], n[0] * cos(y) + n[1] * sin(y))
    r = atan2(a[0] * sin(y) - a[1] * cos(y), -o[0] * sin(y) + o[1] * cos(y))
    return np.array([y, p, r]) / pi * 180.0


def ypr2R(ypr):
    y, p, r = np.asarray(ypr, float) / 180.0 * pi
    Rz = np.array([[cos(y), -sin(y), 0], [sin(y), cos(y), 0], [0, 0, 1]])
    Ry = np.array([[cos(p), 0, sin(p)], [0, 1, 0], [-sin(p), 0, cos(p)]])
    Rx = np.array([[1, 0, 0], [0, cos(r), -sin(r)], [0, sin(r), cos(r)]])
    return Rz @ Ry @ Rx


def normalize_angle(a):
    """Utility::normalizeAngle (degrees)."""
    if a > 0:
        return a - 360.0 * np.floor((a + 180.0) / 360.0)
    return a + 360.0 * np.floor((-a + 180.0) / 360.0)


def relo_tail(rot_diff, origin_P0, para_pose0, relo_pose, prev_relo_t, prev_relo_r, P_frame, R_frame):
    """relo_r, relo_t, drift_correct_yaw / r / t, relo_relative_t / q (as a matrix) / yaw."""
    q = np_ref.pose_q(relo_pose)
    relo_r = rot_diff @ np_ref.qR(q / np.linalg.norm(q))
    relo_t = rot_diff @ (relo_pose[:3] - para_pose0[:3]) + origin_P0
    yaw = R2ypr(prev_relo_r)[0] - R2ypr(relo_r)[0]
    drift_r = ypr2R([yaw, 0, 0])
    drift_t = prev_relo_t - drift_r @ relo_t
    rel_t = relo_r.T @ (P_frame - relo_t)
    rel_R = relo_r.T @ R_frame
    rel_yaw = normalize_angle(R2ypr(R_frame)[0] - R2ypr(relo_r)[0])
    return dict(relo_r=relo_r, relo_t=relo_t, drift_correct_yaw=yaw, drift_correct_r=drift_r, drift_correct_t=drift_t,
                relo_relative_t=rel_t, relo_relative_R=rel_R, relo_relative_yaw=rel_yaw)
