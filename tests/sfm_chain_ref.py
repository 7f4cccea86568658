"""The incremental part of GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:121-218) restated on top of tests/pnp_ref.py:
the reference of tests/test_sfm_chain.py, tests/test_sfm_chain_ref.py and tests/golden/gen_sfm_chain_hp.py, and what
lfvio_sfm_construct (include/lfvio.h) is measured with.

One text for two arithmetics, pnp_ref's F64 and HP (numpy float64, or mpmath at 50 digits; there every input double is taken exactly
and nothing is rounded on the way: a PnP gets the 50-digit positions, not their roundings):

  schedule(F, l)                     the op table: ("pnp", i, i) / ("tri", a, b) / ("close", 0, 0), numbered from 0 in the reference's order
  construct(F, l, off, frame, bearing, relative_R, relative_T, be)

Restated literally: :125-153 (Quaterniond(relative_R) by Eigen's four branches, inverse() = conjugate / squared norm,
toRotationMatrix(), c_Translation = -1 * (c_Rotation * T)); solveFrameByPnP :23-71 (state == true and an observation in frame i, in
ascending j; fewer than 10 returns false) over pnp_ref.compute_pose; triangulateTwoFrames :73-110; triangulatePoint :6-21 (the right
singular vector of the smallest singular value of the 4 x 4 design matrix, divided by its fourth entry); the closing loop :197-218
(first and last observation).  c_Quat[i] = c_Rotation[i] of a PnP result is the same matrix to quaternion conversion, reflection or
not.  The device's deviations are restated too: status 2 where compute_pose's finiteness gate trips, and a chain that stops leaves
the poses of the frames it did not reach unset (NaN here).  Sign pinning is pnp_ref's (pin_axis); a triangulated point does not depend
on the sign of its singular vector.
"""
import numpy as np

import pnp_ref as pr

EPS = 2.0 ** -52
MIN_PNP = 10


def schedule(F, l):
    ops = []
    for i in range(l, F - 1):  # :157-175
        if i > l:
            ops.append(("pnp", i, i))
        ops.append(("tri", i, F - 1))
    for i in range(l + 1, F - 1):  # :177-178
        ops.append(("tri", l, i))
    for i in range(l - 1, -1, -1):  # :181-195
        ops.append(("pnp", i, i))
        ops.append(("tri", i, l))
    ops.append(("close", 0, 0))  # :197-218
    return ops


def quat_of_matrix(m, be):
    """Eigen's Quaternion(Matrix3) -> [w, x, y, z]."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = [be.zero] * 4
    if t > 0:
        t = be.sqrt(t + 1)
        q[0] = t / 2
        t = be.one / 2 / t
        q[1], q[2], q[3] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = be.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        q[1 + i] = t / 2
        t = be.one / 2 / t
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    return np.array(q, dtype=be.dtype)


def quat_mul(a, b, be):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=be.dtype)


def quat_inverse(q, be):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    r = be.one / n2
    return np.array([q[0] * r, -q[1] * r, -q[2] * r, -q[3] * r], dtype=be.dtype)


def matrix_of_quat(q, be):
    """Eigen's toRotationMatrix (no normalisation)."""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype=be.dtype)


def rotation_of(q):
    """R(q / |q|) in double precision for q [..., 4] (w x y z): what the tests compare rotations through (q and -q are one rotation)."""
    q = np.asarray(q, np.float64)
    w, x, y, z = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def design_matrix(P0, P1, u0, u1, be):
    A = np.empty((4, 4), dtype=be.dtype)
    A[0] = u0[0] * P0[2] - u0[2] * P0[0]
    A[1] = u0[1] * P0[2] - u0[2] * P0[1]
    A[2] = u1[0] * P1[2] - u1[2] * P1[0]
    A[3] = u1[1] * P1[2] - u1[2] * P1[1]
    return A


def triangulate_point(P0, P1, u0, u1, be):
    """-> (point [3], the singular values ascending, the fourth entry of the unit singular vector)."""
    _, s, v = be.svd(design_matrix(P0, P1, u0, u1, be))
    order = sorted(range(4), key=lambda i: s[i])
    x = v[:, order[0]]
    return np.array([x[0] / x[3], x[1] / x[3], x[2] / x[3]], dtype=be.dtype), [s[i] for i in order], x[3]


class _HPCarry(pr._HP):
    """pnp_ref.HP for a compute_pose() whose world points are 50-digit numbers already.  compute_pose() converts its inputs to double on
    the way in (for it every input IS a double); arr() hands the unrounded points back for the array that is their rounding."""

    def __init__(self, pws):
        super().__init__()
        self._pws, self._rounded = pws, pr.to_double(pws)

    def arr(self, a):
        a = np.asarray(a)
        if a.shape == self._rounded.shape and np.array_equal(a, self._rounded):
            return self._pws.copy()
        return super().arr(a)


def pnp_conditions(pws, be):
    """What decides the control points of a PnP on these world points: (the eigenvalues of the 3 x 3 moment, ascending; per principal axis
    the ratio of its largest |component| to the second largest)."""
    pws = pws if pws.dtype == be.dtype else be.arr(pws)
    PW0 = pws - pws.sum(0) / len(pws)
    lam, vec = be.eigh(PW0.T.dot(PW0))
    pins = []
    for k in range(3):
        c = sorted((abs(x) for x in vec[:, k]), reverse=True)
        pins.append(c[0] / c[1] if c[1] != 0 else float("inf"))
    return [x for x in lam], pins


def construct(F, l, off, frame, bearing, relative_R, relative_T, be=pr.F64, min_pnp=MIN_PNP):
    """-> dict(status, failed_frame, num_triangulated, pnp_op [F], pnp_count [F], pnp {frame: compute_pose's dict}, c_rotation [F, 4]
    (w x y z), c_translation [F, 3], R [F, 3, 3] (c_Rotation), position [P, 3], tri_op [P], posed [F], and for the generator's conditions
    tri_sv {j: singular values ascending}, tri_w {j: fourth entry}, pnp_cond {frame: pnp_conditions()}) in the arithmetic of `be`."""
    off, frame = np.asarray(off, np.int64), np.asarray(frame, np.int64)
    P = len(off) - 1
    us = be.arr(np.asarray(bearing, np.float64).reshape(-1, 3))
    slot = -np.ones((P, F), np.int64)
    for j in range(P):
        for o in range(off[j], off[j + 1]):
            assert 0 <= frame[o] < F and slot[j, frame[o]] < 0
            slot[j, frame[o]] = o
    nan = be.num(float("nan"))
    cq, ct, cR = np.full((F, 4), nan, dtype=be.dtype), np.full((F, 3), nan, dtype=be.dtype), np.full((F, 3, 3), nan, dtype=be.dtype)
    pose = [None] * F
    posed = np.zeros(F, bool)

    def set_pose(f, q, R, t):
        cq[f], cR[f], ct[f] = q, R, t
        pose[f] = np.concatenate([R, t.reshape(3, 1)], 1)
        posed[f] = True

    # :125-153
    q_l = np.array([be.one, be.zero, be.zero, be.zero], dtype=be.dtype)
    q_n = quat_mul(q_l, quat_of_matrix(be.arr(np.asarray(relative_R, np.float64).reshape(3, 3)), be), be)
    for f, q, T in ((l, q_l, be.arr(np.zeros(3))), (F - 1, q_n, be.arr(np.asarray(relative_T, np.float64).reshape(3)))):
        c_quat = quat_inverse(q, be)
        R = matrix_of_quat(c_quat, be)
        set_pose(f, c_quat, R, -R.dot(T))

    X = np.full((P, 3), be.zero, dtype=be.dtype)
    tri_op = -np.ones(P, np.int64)
    pnp_op, pnp_count = -np.ones(F, np.int64), np.zeros(F, np.int64)
    pnp, tri_sv, tri_w, pnp_cond = {}, {}, {}, {}
    status, failed = 0, -1
    for op, (kind, a, b) in enumerate(schedule(F, l)):
        if kind == "pnp":
            js = [j for j in range(P) if tri_op[j] >= 0 and slot[j, a] >= 0]
            pnp_op[a], pnp_count[a] = op, len(js)
            if len(js) < min_pnp:
                status, failed = 1, a
                break
            pws, u = X[js], us[[slot[j, a] for j in js]]
            if be is pr.F64:
                with np.errstate(all="ignore"):
                    res = pr.compute_pose(pws, u)
            else:
                res = pr.compute_pose(pr.to_double(pws), pr.to_double(u), _HPCarry(pws))
            pnp[a] = res
            if res["status"] != 0:
                status, failed = 2, a
                break
            pnp_cond[a] = pnp_conditions(pws, be)
            R = np.array(res["R"], dtype=be.dtype)
            set_pose(a, quat_of_matrix(R, be), R, np.array(res["T"], dtype=be.dtype))
        else:
            for j in range(P):
                if tri_op[j] >= 0:
                    continue
                if kind == "tri":
                    o0, o1, f0, f1 = slot[j, a], slot[j, b], a, b
                else:
                    s, e = off[j], off[j + 1]
                    o0, o1, f0, f1 = (s if e - s >= 2 else -1), e - 1, frame[s], frame[e - 1]
                if o0 < 0 or o1 < 0:
                    continue
                with np.errstate(all="ignore"):
                    X[j], tri_sv[j], tri_w[j] = triangulate_point(pose[f0], pose[f1], us[o0], us[o1], be)
                tri_op[j] = op
    return dict(status=status, failed_frame=failed, num_triangulated=int((tri_op >= 0).sum()), pnp_op=pnp_op, pnp_count=pnp_count, pnp=pnp, c_rotation=cq,
                c_translation=ct, R=cR, position=X, tri_op=tri_op, posed=posed, tri_sv=tri_sv, tri_w=tri_w, pnp_cond=pnp_cond)


def compact(res, off, frame, bearing):
    """The hand-over to the bundle adjustment (:259-275): the points with tri_op >= 0, in order, with their observations, as a CSR."""
    off = np.asarray(off, np.int64)
    keep = np.nonzero(np.asarray(res["tri_op"]) >= 0)[0]
    obs = np.concatenate([np.arange(off[j], off[j + 1]) for j in keep]) if len(keep) else np.zeros(0, np.int64)
    o2 = np.concatenate([[0], np.cumsum(np.diff(off)[keep])]).astype(np.int32)
    return dict(keep=keep, off=o2, frame=np.asarray(frame, np.int32)[obs], bearing=np.asarray(bearing, np.float64).reshape(-1, 3)[obs],
                position=np.asarray(res["position"], np.float64)[keep])
