"""PnpSolver::compute_pose (vins_estimator/src/pnp_solver.cpp) restated: the reference of tests/test_pnp.py, tests/test_pnp_host.py
and tests/golden/gen_pnp_hp.py.  Internal parameters are the reference's only call form, (cx, cy, fx, fy) = (0, 0, 1, 1).

One text for two arithmetics (numpy arrays of float64, or of mpmath numbers at 50 digits):

  compute_pose(pws, us)       double precision — what the device is also measured with (bar = 16 x this one's error)
  compute_pose(pws, us, HP)   50 digits; every input is a double and is taken exactly, nothing is rounded before the end;
                              used by the generator and by the one CPU test that ties the file to it

Restated literally (line numbers of pnp_solver.cpp): choose_control_points :45-75, compute_barycentric_coordinates :76-96, M
:313-325, M^T M and its four smallest singular vectors :326-333, compute_L_6x10 :101-135, compute_rho :136-144, find_betas_*
:145-230 (B5[0] = -B5[0] of :226-227 is a dead store and stays one), gauss_newton :388-440 (15 steps), compute_ccs / pcs
:231-245, solve_for_sign :246-254 (first correspondence only), estimate_R_and_t :255-284 (no determinant fix),
reprojection_error :285-296, the winner :355-369.  colPivHouseholderQr().solve is Eigen's (ColPivHouseholderQR.h: column
norms with downdating, the rank threshold on the largest remaining column norm, zeros for the dropped components).
Not pinned: the signs an SVD gives its null vectors and the vectors of W (numpy's / mpmath's here, Eigen's in the reference,
the device's own).  Pinned by a rule of this project's own, pin_axis(): the signs of the principal axes behind the control points.
"""
import numpy as np

EPS = 2.0 ** -52


class F64:
    """double precision"""
    dtype = np.float64
    zero, one = 0.0, 1.0
    eps, tiny = EPS, 2.2250738585072014e-308

    @staticmethod
    def num(x):
        return float(x)

    @staticmethod
    def arr(a):
        return np.array(a, dtype=np.float64)

    sqrt = staticmethod(lambda x: float(np.sqrt(x)) if x >= 0 else float("nan"))

    @staticmethod
    def eigh(A):
        """Eigenvalues ascending, eigenvectors in columns."""
        w, v = np.linalg.eigh(A)
        return w, v

    @staticmethod
    def svd(A):
        u, s, vt = np.linalg.svd(A)
        return u, s, vt.T

    @staticmethod
    def finite(x):
        return bool(np.isfinite(x))


class _HP:
    """mpmath at hp_ref.DPS digits (imported on first use: the GPU tests never need mpmath)"""
    dtype = object
    tiny = 0

    def __init__(self):
        self._mp = None

    @property
    def mp(self):
        if self._mp is None:
            import hp_ref  # sets the precision

            self._mp = hp_ref.mp
        return self._mp

    @property
    def zero(self):
        return self.mp.mpf(0)

    @property
    def one(self):
        return self.mp.mpf(1)

    @property
    def eps(self):
        return self.mp.mpf(2) ** -52  # (the rank threshold of the solve is part of what is restated: Eigen's, for doubles)

    def num(self, x):
        return self.mp.mpf(float(x)) if not isinstance(x, self.mp.mpf) else x

    def arr(self, a):
        a = np.asarray(a)
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            out[idx] = self.num(a[idx])
        return out

    def sqrt(self, x):
        return self.mp.sqrt(x) if x >= 0 else self.mp.nan

    def eigh(self, A):
        n = A.shape[0]
        E, Q = self.mp.eigsy(self.mp.matrix(A.tolist()))
        order = sorted(range(n), key=lambda i: E[i])
        return np.array([E[i] for i in order], dtype=object), np.array([[Q[r, i] for i in order] for r in range(n)], dtype=object)

    def svd(self, A):
        n = A.shape[0]
        U, S, V = self.mp.svd_r(self.mp.matrix(A.tolist()), full_matrices=True, compute_uv=True)  # A = U diag(S) V, V rows
        u = np.array([[U[r, c] for c in range(n)] for r in range(n)], dtype=object)
        v = np.array([[V[c, r] for c in range(n)] for r in range(n)], dtype=object)
        return u, np.array([S[i] for i in range(n)], dtype=object), v

    def finite(self, x):
        return bool(self.mp.isfinite(x))


HP = _HP()


def colpiv_solve(A, b, be):
    """A.colPivHouseholderQr().solve(b), Eigen 3.3/3.4 (computeInPlace, _solve_impl)."""
    A, b = A.copy(), b.copy()
    rows, cols = A.shape
    size = min(rows, cols)
    nu = [be.sqrt(sum(A[r, c] * A[r, c] for r in range(rows))) for c in range(cols)]
    nd = list(nu)
    perm = list(range(cols))
    hc = [be.zero] * size
    thr_helper = (max(nu) * be.eps) * (max(nu) * be.eps) / rows
    downdate = be.sqrt(be.eps)
    nonzero = size
    for k in range(size):
        big = max(range(k, cols), key=lambda c: (nu[c], -c))  # maxCoeff: the first of equal ones
        if nonzero == size and nu[big] * nu[big] < thr_helper * (rows - k):
            nonzero = k
        if big != k:
            A[:, [k, big]] = A[:, [big, k]]
            nu[k], nu[big], nd[k], nd[big], perm[k], perm[big] = nu[big], nu[k], nd[big], nd[k], perm[big], perm[k]
        tail = sum((A[r, k] * A[r, k] for r in range(k + 1, rows)), be.zero)
        c0 = A[k, k]
        if tail <= be.tiny:
            tau, beta = be.zero, c0
            for r in range(k + 1, rows):
                A[r, k] = be.zero
        else:
            beta = be.sqrt(c0 * c0 + tail)
            if c0 >= 0:
                beta = -beta
            for r in range(k + 1, rows):
                A[r, k] = A[r, k] / (c0 - beta)
            tau = (beta - c0) / beta
        A[k, k], hc[k] = beta, tau
        for c in range(k + 1, cols):
            t = A[k, c] + sum((A[r, k] * A[r, c] for r in range(k + 1, rows)), be.zero)
            A[k, c] = A[k, c] - tau * t
            for r in range(k + 1, rows):
                A[r, c] = A[r, c] - tau * A[r, k] * t
        for c in range(k + 1, cols):
            if nu[c] != 0:
                t = abs(A[k, c]) / nu[c]
                t = (1 + t) * (1 - t)
                t = be.zero if t < 0 else t
                q = nu[c] / nd[c]
                if t * (q * q) <= downdate:
                    nd[c] = be.sqrt(sum((A[r, c] * A[r, c] for r in range(k + 1, rows)), be.zero))
                    nu[c] = nd[c]
                else:
                    nu[c] = nu[c] * be.sqrt(t)
    for k in range(nonzero):
        t = b[k] + sum((A[r, k] * b[r] for r in range(k + 1, rows)), be.zero)
        b[k] = b[k] - hc[k] * t
        for r in range(k + 1, rows):
            b[r] = b[r] - hc[k] * A[r, k] * t
    y = [be.zero] * cols
    for i in range(nonzero - 1, -1, -1):
        s = b[i]
        for c in range(i + 1, nonzero):
            s = s - A[i, c] * y[c]
        y[i] = s / A[i, i]
    x = np.array([be.zero] * cols, dtype=be.dtype)
    for i in range(nonzero):
        x[perm[i]] = y[i]
    return x


def _pairs():
    return [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def compute_L_6x10(ut, be):
    dv = [[ut[i][3 * a:3 * a + 3] - ut[i][3 * b:3 * b + 3] for (a, b) in _pairs()] for i in range(4)]
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    L = np.empty((6, 10), dtype=be.dtype)
    for i in range(6):
        L[i] = [dot(dv[0][i], dv[0][i]), 2 * dot(dv[0][i], dv[1][i]), dot(dv[1][i], dv[1][i]), 2 * dot(dv[0][i], dv[2][i]),
                2 * dot(dv[1][i], dv[2][i]), dot(dv[2][i], dv[2][i]), 2 * dot(dv[0][i], dv[3][i]), 2 * dot(dv[1][i], dv[3][i]),
                2 * dot(dv[2][i], dv[3][i]), dot(dv[3][i], dv[3][i])]
    return L


def find_betas(which, L, rho, be):
    B = colpiv_solve(L[:, [[0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4]][which]], rho, be)
    z = be.zero
    if which == 0:
        if B[0] < 0:
            b0 = be.sqrt(-B[0])
            return [b0, -B[1] / b0, -B[2] / b0, -B[3] / b0]
        b0 = be.sqrt(B[0])
        return [b0, B[1] / b0, B[2] / b0, B[3] / b0]
    if B[0] < 0:
        b0, b1 = be.sqrt(-B[0]), (be.sqrt(-B[2]) if B[2] < 0 else z)
    else:
        b0, b1 = be.sqrt(B[0]), (be.sqrt(B[2]) if B[2] > 0 else z)
    if which == 1:
        if B[1] < 0:
            b0 = -b0
        return [b0, b1, z, z]
    return [b0, b1, B[3] / b0, z]  # (:226-227 negates B5[0] after its last use)


def gauss_newton(L, rho, betas, be):
    b = list(betas)
    for _ in range(15):
        A, r = np.empty((6, 4), dtype=be.dtype), np.empty(6, dtype=be.dtype)
        for i in range(6):
            l = L[i]
            A[i, 0] = 2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3]
            A[i, 1] = l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3]
            A[i, 2] = l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3]
            A[i, 3] = l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3]
            r[i] = rho[i] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] +
                             l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3])
        x = colpiv_solve(A, r, be)
        b = [b[i] + x[i] for i in range(4)]
    return b


def pin_axis(v):
    """The sign of a principal axis of the world points: its largest component (the first of equal ones) positive.  The
    control points depend on these signs, and with noisy bearings the pose depends on the control points at the level of the
    noise (1e-2 in R at 1 px, f = 160), so an SVD's own choice cannot be left open here as it can for the other vectors."""
    k = int(np.argmax([abs(x) for x in v]))
    return -v if v[k] < 0 else v


def compute_pose(pws, us, be=F64):
    """-> dict(status, chosen, R [3, 3], T [3], err [3], R_all [3, 3, 3], T_all [3, 3]) in the arithmetic of `be`; status 1 (a
    non-finite value among the errors or the winner's pose) is the device's deviation from the reference, restated."""
    pws, us = be.arr(np.asarray(pws, np.float64).reshape(-1, 3)), be.arr(np.asarray(us, np.float64).reshape(-1, 3))
    n = len(pws)
    nan = float("nan")
    try:
        c0 = pws.sum(0) / n
        PW0 = pws - c0
        lam, vec = be.eigh(PW0.T.dot(PW0))  # JacobiSVD of a symmetric positive semidefinite matrix: U = its eigenvectors
        cws = np.empty((4, 3), dtype=be.dtype)
        cws[0] = c0
        for i in range(1, 4):
            cws[i] = c0 + be.sqrt(lam[3 - i] / n) * pin_axis(vec[:, 3 - i])
        CC = (cws[1:] - cws[0]).T
        a = [[CC[1, 1] * CC[2, 2] - CC[1, 2] * CC[2, 1], CC[0, 2] * CC[2, 1] - CC[0, 1] * CC[2, 2], CC[0, 1] * CC[1, 2] - CC[0, 2] * CC[1, 1]],
             [CC[1, 2] * CC[2, 0] - CC[1, 0] * CC[2, 2], CC[0, 0] * CC[2, 2] - CC[0, 2] * CC[2, 0], CC[0, 2] * CC[1, 0] - CC[0, 0] * CC[1, 2]],
             [CC[1, 0] * CC[2, 1] - CC[1, 1] * CC[2, 0], CC[0, 1] * CC[2, 0] - CC[0, 0] * CC[2, 1], CC[0, 0] * CC[1, 1] - CC[0, 1] * CC[1, 0]]]
        det = CC[0, 0] * a[0][0] + CC[0, 1] * a[1][0] + CC[0, 2] * a[2][0]
        if det == 0 or not be.finite(det):
            raise ZeroDivisionError
        CI = np.array(a, dtype=be.dtype) / det
        alphas = np.empty((n, 4), dtype=be.dtype)
        alphas[:, 1:] = PW0.dot(CI.T)
        alphas[:, 0] = 1 - alphas[:, 1] - alphas[:, 2] - alphas[:, 3]
        if np.any(us[:, 2] == 0):
            raise ZeroDivisionError
        M = np.empty((2 * n, 12), dtype=be.dtype)
        M[:] = be.zero
        for j in range(4):
            M[0::2, 3 * j] = alphas[:, j]
            M[0::2, 3 * j + 2] = alphas[:, j] * (0 - us[:, 0]) / us[:, 2]
            M[1::2, 3 * j + 1] = alphas[:, j]
            M[1::2, 3 * j + 2] = alphas[:, j] * (0 - us[:, 1]) / us[:, 2]
        w, v = be.eigh(M.T.dot(M))
        ut = [v[:, i] for i in range(4)]  # Ut(11 - i): the i-th smallest
        L = compute_L_6x10(ut, be)
        rho = np.array([sum((cws[a_] - cws[b_]) ** 2) for (a_, b_) in _pairs()], dtype=be.dtype)
        Rs, Ts, errs = [], [], []
        pw0 = c0
        for which in range(3):
            betas = gauss_newton(L, rho, find_betas(which, L, rho, be), be)
            ccs = np.array([[sum(betas[i] * ut[i][3 * j + k] for i in range(4)) for k in range(3)] for j in range(4)], dtype=be.dtype)
            pcs = alphas.dot(ccs)
            sign0 = 1 if us[0, 2] > 0 else -1
            if (pcs[0, 2] < 0 and sign0 > 0) or (pcs[0, 2] > 0 and sign0 < 0):
                ccs, pcs = -ccs, -pcs
            pc0 = pcs.sum(0) / n
            W = (pcs - pc0).T.dot(pws - pw0)
            U, _, V = be.svd(W)
            R = U.dot(V.T)
            T = pc0 - R.dot(pw0)
            d = us - (pws.dot(R.T) + T)
            errs.append((d * d).sum() / n)
            Rs.append(R), Ts.append(T)
        N = 0
        if errs[1] < errs[0]:
            N = 1
        if errs[2] < errs[N]:
            N = 2
        ok = all(be.finite(e) for e in errs) and all(be.finite(x) for x in Rs[N].reshape(-1)) and all(be.finite(x) for x in Ts[N])
    except (ZeroDivisionError, FloatingPointError, np.linalg.LinAlgError):
        ok = False
    if not ok:
        return dict(status=1, chosen=-1, R=np.full((3, 3), nan), T=np.full(3, nan), err=np.full(3, nan), R_all=np.full((3, 3, 3), nan), T_all=np.full((3, 3), nan))
    return dict(status=0, chosen=N, R=Rs[N], T=Ts[N], err=np.array(errs, dtype=be.dtype), R_all=np.array(Rs, dtype=be.dtype), T_all=np.array(Ts, dtype=be.dtype))


def to_double(x):
    return np.array(x, dtype=object).astype(np.float64) if isinstance(x, np.ndarray) else float(x)


def pnp(offset, point_w, bearing):
    """The batched call in double precision: a list of compute_pose() results, one per frame of the CSR."""
    pw, us = np.asarray(point_w, np.float64).reshape(-1, 3), np.asarray(bearing, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return [compute_pose(pw[offset[f]:offset[f + 1]], us[offset[f]:offset[f + 1]]) for f in range(len(offset) - 1)]


def post_process(R_pnp, T_pnp, ric):
    """estimator.cpp:353-356: R_pnp^T, then T = R_pnp^T (-T_pnp) and ImageFrame::R = R_pnp^T RIC^T, ImageFrame::T = T."""
    Rt = np.asarray(R_pnp).T
    return Rt @ np.asarray(ric).T, Rt @ (-np.asarray(T_pnp))
