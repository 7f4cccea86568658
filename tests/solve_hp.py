"""50-digit statement of the Gauss-Newton step of one trust-region pass (test infrastructure: mpmath and numpy), the reference
that tests/test_solve_hp.py holds k_solve_dense (csrc/kernels_solve.h) and the Schur phase of the landmark sweep to.

Written from Ceres 1.12's formulas as oracle/oracle_solver.cpp (schur_solve, the ComputeStep part of solve) and tests/np_ref.py
(solve) state them — not from the kernel:

  scale_i      = 1 / (1 + sqrt(H_ii))                         jacobi_scaling, iteration 0
  diagonal_i   = sqrt(clip(scale_i^2 H_ii, 1e-6, 1e32))       min / max_lm_diagonal
  gradient_i   = scale_i g_i / diagonal_i                     0 in a constant column
  landmarks    e_l = s_l^2 a_l + mu d_l^2,  c_l = s_l^2 / e_l
               C = sum c_l w_l w_l^T,  z1 = sum c_l b_l w_l                         the elimination
               z2 = sum (s_l^2 b_l / d_l^2) w_l,  ls1 = sum gradient_l^2,  ls2 = sum a_l (s_l^2 b_l / d_l^2)^2   the Cauchy point
  S            = s (H - C) s + mu D^2,  rhs = s (g - z1);  identity rows and a zero rhs in constant columns
  S y = rhs;   gauss_newton_step_ = -D y;  G = s gradient_ / D,  N = -s y  (the unscaled directions)
  alpha        = (|gradient_|^2 + ls1) / (G^T H G + 2 z2 . G_c + ls2)
  Q_GG, Q_GN, Q_NN = G^T H G, G^T H N, N^T H N  as x^T H x over the full matrix;  Q_gG, Q_gN = g . G, g . N;
  Q_GRAD_SQ, Q_GN_SQ, Q_GRAD_GN = |gradient_|^2, |gauss_newton_step_|^2, gradient_ . gauss_newton_step_   (pose side)

Every input is a double and is taken exactly; mpmath numbers travel in numpy object arrays and are rounded by the caller.
The bars at the end of the file are 16 x the worst value that three double-precision solvers show over the case list of
tests/test_solve_hp.py — measured on the CPU, never on the kernel.
"""
import mpmath as mp
import numpy as np

import np_ref

DPS = 50
mp.mp.dps = DPS
KC, KP = np_ref.KC, np_ref.KP
EPS = 2.0 ** -53
MIN_DIAG, MAX_DIAG = 1e-6, 1e32  # min_lm_diagonal, max_lm_diagonal
CERTIFICATE = 1e-40
# indices of TRState::q (csrc/dev_types.h)
Q_NAMES = ("Q_GG", "Q_GN", "Q_NN", "Q_gG", "Q_gN", "Q_GRAD_SQ", "Q_GN_SQ", "Q_GRAD_GN")
Q_WITHOUT_Y = ("Q_GG", "Q_gG", "Q_GRAD_SQ")


def to_mp(a):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.size, dtype=object)
    for i, v in enumerate(a.ravel()):
        out[i] = mp.mpf(float(v))
    return out.reshape(a.shape)


def to_f(a):
    a = np.asarray(a, dtype=object)
    return np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def _dot(a, b):
    return mp.fdot(list(a), list(b))


def _matvec(rows, x):
    """rows: a list of lists of mpf (prepared once per matrix)."""
    xl = list(x)
    out = np.empty(len(rows), dtype=object)
    for i, r in enumerate(rows):
        out[i] = mp.fdot(r, xl)
    return out


def _clip(x):
    return min(max(x, mp.mpf(MIN_DIAG)), mp.mpf(MAX_DIAG))


def active_columns(est_ex, est_td):
    act = np.ones(KP, dtype=bool)
    if not est_ex:
        act[np_ref.OFF_EX:np_ref.OFF_EX + 6] = False
    if not est_td:
        act[np_ref.OFF_TD] = False
    return act


def imu_columns(f):
    """Tangent columns of IMU factor f's 30 x 30 block, [pose_f | sb_f | pose_f+1 | sb_f+1]."""
    return ([np_ref.off_pose(f) + k for k in range(6)] + [np_ref.off_sb(f) + k for k in range(9)]
            + [np_ref.off_pose(f + 1) + k for k in range(6)] + [np_ref.off_sb(f + 1) + k for k in range(9)])


def prior_column_map(prior):
    """prior column -> tangent column, from the prior's block list (kind, frame, first column of the block)."""
    cmap = np.full(prior.n, -1, dtype=np.int64)
    for i in range(prior.num_blocks):
        kind, frame, idx = prior.blocks[i].kind, prior.blocks[i].frame, prior.block_idx[i]
        for k in range(np_ref.block_local(kind)):
            cmap[idx + k] = np_ref.block_off(kind, frame) + k
    assert (cmap >= 0).all() and len(set(cmap.tolist())) == prior.n
    return cmap


def packed_lower(Hp, rows=KP):
    """[rows, rows] symmetric matrix of the packed lower triangle (entry (i, j <= i) at i (i + 1) / 2 + j)."""
    H = np.zeros((rows, rows))
    for i in range(rows):
        H[i, :i + 1] = Hp[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1]
    return H + np.tril(H, -1).T


def assemble_hp(vis, imu_blocks, prior_A, prior_cmap, est_ex, est_td):
    """H_pp from the three sources of the assembling solve: vis [73, 73] the visual terms of the camera part; imu_blocks
    [10][30, 30] (a skipped factor: zeros); prior_A [n, n] = J0^T J0 with its column map.  Entry (i, j <= i) of H takes, of every
    source, the entry at (row of tangent column i, column of tangent column j) — nothing else of a source is read (the sweep of a
    resident batch stores no more of an IMU block) — and the columns of a constant ex / td are taken out.  Object array [172, 172]."""
    H = to_mp(np.zeros((KP, KP)))
    V = to_mp(vis)
    for i in range(KC):
        for j in range(i + 1):
            H[i, j] = V[i, j]
    for f in range(10):
        cols = imu_columns(f)
        B = to_mp(imu_blocks[f])
        for p in range(30):
            for q in range(30):
                i, j = cols[p], cols[q]
                if i >= j:
                    H[i, j] += B[p, q]
    n = len(prior_cmap)
    if n:
        A = to_mp(prior_A)
        for p in range(n):
            for q in range(n):
                i, j = int(prior_cmap[p]), int(prior_cmap[q])
                if i >= j:
                    H[i, j] += A[p, q]
    act = active_columns(est_ex, est_td)
    zero = mp.mpf(0)
    for i in range(KP):
        for j in range(i + 1):
            if not (act[i] and act[j]):
                H[i, j] = zero
            H[j, i] = H[i, j]
    return H


def schur_hp(a, b, W, mu):
    """The landmark elimination at iteration 0.  Returns C [73, 73], z1, z2 [73], ls1, ls2 (mpf in object arrays) and, under the
    same names with the prefix `abs_`, the sum of the absolute values of the terms of every entry (doubles: they are units)."""
    a, b, W = np.asarray(a, float), np.asarray(b, float), np.asarray(W, float).reshape(-1, KC)
    N = len(a)
    zero, mu_ = mp.mpf(0), mp.mpf(float(mu))
    C = to_mp(np.zeros((KC, KC)))
    z1, z2 = to_mp(np.zeros(KC)), to_mp(np.zeros(KC))
    ls1 = ls2 = zero
    cf, kf, s2f, d2f = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for l in range(N):
        al, bl = mp.mpf(float(a[l])), mp.mpf(float(b[l]))
        s = 1 / (1 + mp.sqrt(al))
        s2a = s * s * al
        d2 = _clip(s2a)
        c = s * s / (s2a + mu_ * d2)
        kappa = s * s * bl / d2  # the landmark's entry of scale * gradient_ / diagonal_
        ls1 += s * s * bl * bl / d2
        ls2 += al * kappa * kappa
        cf[l], kf[l], s2f[l], d2f[l] = float(c), float(kappa), float(s * s), float(d2)
        nz = np.nonzero(W[l])[0]
        w = [mp.mpf(float(W[l, k])) for k in nz]
        cw = [c * x for x in w]
        cb = c * bl
        for p, i in enumerate(nz):
            z1[i] += cb * w[p]
            z2[i] += kappa * w[p]
            cwp = cw[p]
            for q in range(p + 1):
                C[i, nz[q]] += cwp * w[q]
    for i in range(KC):
        for j in range(i):
            C[j, i] = C[i, j]
    aW = np.abs(W)
    return dict(C=C, z1=z1, z2=z2, ls1=ls1, ls2=ls2,
                abs_C=(aW * cf[:, None]).T @ aW, abs_z1=(cf * np.abs(b)) @ aW, abs_z2=np.abs(kf) @ aW,
                abs_ls1=float(np.sum(s2f * b * b / d2f)) if N else 0.0, abs_ls2=float(np.sum(a * kf * kf)) if N else 0.0)


def schur_double(a, b, W, mu, order=None):
    """The same sums as a plain numpy evaluation in double, landmark by landmark in `order` (a comparator)."""
    a, b, W = np.asarray(a, float), np.asarray(b, float), np.asarray(W, float).reshape(-1, KC)
    C, z1, z2, ls1, ls2 = np.zeros((KC, KC)), np.zeros(KC), np.zeros(KC), 0.0, 0.0
    for l in (range(len(a)) if order is None else order):
        s = 1.0 / (1.0 + np.sqrt(a[l]))
        d2 = min(max(s * s * a[l], MIN_DIAG), MAX_DIAG)
        c = s * s / (s * s * a[l] + mu * d2)
        kappa = s * s * b[l] / d2
        C += c * np.outer(W[l], W[l])
        z1 += (c * b[l]) * W[l]
        z2 += kappa * W[l]
        gr = s * b[l] / np.sqrt(d2)
        ls1 += gr * gr
        ls2 += a[l] * kappa * kappa
    return dict(C=C, z1=z1, z2=z2, ls1=ls1, ls2=ls2)


def schur_report(got, hp):
    """|got - hp| over the sum of the absolute terms of the entry, in units of eps: the worst entry of C, z1, z2 and the scalars.
    An entry without terms must be exactly zero (inf otherwise)."""
    rep = {}
    for k in ("C", "z1", "z2", "ls1", "ls2"):
        g = np.asarray(got[k], dtype=np.float64).reshape(-1)
        h = np.asarray(hp[k], dtype=object).reshape(-1)
        den = np.asarray(hp["abs_" + k], dtype=np.float64).reshape(-1)
        worst = 0.0
        for i in range(g.size):
            d = abs(float(mp.mpf(float(g[i])) - h[i]))
            if den[i] > 0:
                worst = max(worst, d / den[i] / EPS)
            elif d != 0:
                worst = np.inf
        rep[k] = worst
    return rep


def reduced_hp(H, g, C, z1, mu, active):
    """scale, diagonal_, gradient_, the scaled reduced system S (identity rows in inactive columns) and its rhs.
    H [172, 172], g [172], C [73, 73], z1 [73]: doubles or mpf; object arrays out."""
    H, g = np.asarray(H, dtype=object), np.asarray(g, dtype=object)
    mpf = lambda x: x if isinstance(x, mp.mpf) else mp.mpf(float(x))  # noqa: E731
    mu_ = mp.mpf(float(mu))
    scale, diag, grad = np.empty(KP, object), np.empty(KP, object), np.empty(KP, object)
    for i in range(KP):
        hii = mpf(H[i, i])
        scale[i] = 1 / (1 + mp.sqrt(hii))
        diag[i] = mp.sqrt(_clip(scale[i] * scale[i] * hii))
        grad[i] = scale[i] * mpf(g[i]) / diag[i] if active[i] else mp.mpf(0)
    S, rhs = np.empty((KP, KP), object), np.empty(KP, object)
    zero, one = mp.mpf(0), mp.mpf(1)
    for i in range(KP):
        for j in range(i + 1):
            if active[i] and active[j]:
                h = mpf(H[i, j])
                if i < KC:
                    h = h - mpf(C[i, j])
                v = scale[i] * h * scale[j]
                if i == j:
                    v += mu_ * diag[i] * diag[i]
            else:
                v = one if i == j else zero
            S[i, j] = S[j, i] = v
        r = mpf(g[i])
        if i < KC:
            r = r - mpf(z1[i])
        rhs[i] = scale[i] * r if active[i] else zero
    return dict(scale=scale, diag=diag, grad=grad, S=S, rhs=rhs, active=np.asarray(active, bool))


def reduced_double(H, g, C, z1, mu, active):
    """The same in double (what the double-precision comparators factor)."""
    H, g = np.asarray(H, float), np.asarray(g, float)
    act = np.asarray(active, bool)
    hd = np.diag(H)
    scale = 1.0 / (1.0 + np.sqrt(hd))
    diag = np.sqrt(np.clip(scale * scale * hd, MIN_DIAG, MAX_DIAG))
    grad = np.where(act, scale * g / diag, 0.0)
    Hr, r = H.copy(), g.copy()
    Hr[:KC, :KC] -= np.asarray(C, float)
    r[:KC] -= np.asarray(z1, float)
    S = scale[:, None] * Hr * scale[None, :] + np.diag(mu * diag * diag)
    S[~act, :] = 0.0
    S[:, ~act] = 0.0
    S[~act, ~act] = 1.0
    return dict(scale=scale, diag=diag, grad=grad, S=S, rhs=np.where(act, scale * r, 0.0), active=act)


def solve_hp(S, rhs):
    """y of S y = rhs to 50 digits, certified: a LAPACK Cholesky factor of the double S, then iterative refinement on the 50-digit
    residual until  |S y - rhs| / (|S|_F |y| + |rhs|) < 1e-40  (asserted: refinement converges only where kappa eps < 1).
    Returns (y, certificate, refinement steps).  numpy.linalg.LinAlgError if the double S does not factor."""
    import scipy.linalg as sl

    Sd, rd = to_f(S), to_f(rhs)
    cf = sl.cho_factor(Sd, lower=True)
    rows = [list(r) for r in S]
    y = to_mp(sl.cho_solve(cf, rd))
    nS, nr = mp.mpf(float(np.linalg.norm(Sd))), mp.sqrt(_dot(rhs, rhs))
    cert = mp.inf
    for step in range(60):
        res = rhs - _matvec(rows, y)
        den = nS * mp.sqrt(_dot(y, y)) + nr
        cert = mp.sqrt(_dot(res, res)) / den if den > 0 else mp.mpf(0)
        if cert < CERTIFICATE:
            return y, float(cert), step
        y = y + to_mp(sl.cho_solve(cf, to_f(res)))
    raise AssertionError(f"solve_hp: no certificate, residual {float(cert):.2e} after 60 refinement steps")


def kappa2(Sd):
    """kappa_2 of the double S (numpy eigvalsh): a unit, three digits suffice."""
    lam = np.linalg.eigvalsh(np.asarray(Sd, float))
    return float(lam[-1] / lam[0]) if lam[0] > 0 else np.inf


def model_hp(H, g, red, y, sch):
    """Everything the dogleg model takes from the step, at the 50-digit y; the quadratic forms as x^T H x over the full matrix.
    sch: schur_hp's dict (ls1, ls2, z2).  Returns a dict of mpf / object arrays."""
    Hm = np.asarray(H, dtype=object)
    if not isinstance(Hm[0, 0], mp.mpf):
        Hm = to_mp(H)
    gm = np.asarray(g, dtype=object)
    if not isinstance(gm[0], mp.mpf):
        gm = to_mp(g)
    s, D, gr = red["scale"], red["diag"], red["grad"]
    G = s * gr / D
    Nn = -(s * y)
    gn = -(D * y)
    rows = [list(r) for r in Hm]
    HG, HN = _matvec(rows, G), _matvec(rows, Nn)
    out = dict(gn=gn, G=G, N=Nn, Q_GG=_dot(G, HG), Q_GN=_dot(G, HN), Q_NN=_dot(Nn, HN), Q_gG=_dot(gm, G), Q_gN=_dot(gm, Nn),
               Q_GRAD_SQ=_dot(gr, gr), Q_GN_SQ=_dot(gn, gn), Q_GRAD_GN=_dot(gr, gn))
    out["grad_sq_total"] = out["Q_GRAD_SQ"] + sch["ls1"]
    out["alpha"] = out["grad_sq_total"] / (out["Q_GG"] + 2 * _dot(sch["z2"], G[:KC]) + sch["ls2"])
    return out


def model_double(H, g, red, y, sch):
    """The same in double from a double y (the comparators' scalars).  red: reduced_double's dict; sch: ls1, ls2, z2 in double."""
    H, g = np.asarray(H, float), np.asarray(g, float)
    s, D, gr = red["scale"], red["diag"], red["grad"]
    G, Nn, gn = s * gr / D, -(s * y), -(D * y)
    HG, HN = H @ G, H @ Nn
    out = dict(gn=gn, G=G, N=Nn, Q_GG=G @ HG, Q_GN=G @ HN, Q_NN=Nn @ HN, Q_gG=g @ G, Q_gN=g @ Nn, Q_GRAD_SQ=gr @ gr, Q_GN_SQ=gn @ gn,
               Q_GRAD_GN=gr @ gn)
    out["grad_sq_total"] = out["Q_GRAD_SQ"] + float(sch["ls1"])
    out["alpha"] = out["grad_sq_total"] / (out["Q_GG"] + 2.0 * (to_f(sch["z2"]) @ G[:KC]) + float(sch["ls2"]))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# double-precision comparators of the solve
# ------------------------------------------------------------------------------------------------------------------------
def lapack_solve(S, rhs):
    L = np.linalg.cholesky(S)
    import scipy.linalg as sl

    return sl.solve_triangular(L.T, sl.solve_triangular(L, rhs, lower=True), lower=False)


def textbook_solve(S, rhs, rcp=None, bad_pivot=-1, bad_rel=0.0):
    """Unblocked Cholesky (column by column), forward and back substitution.  rcp: the reciprocal the column scaling uses (default a
    division); bad_pivot, bad_rel: that pivot's reciprocal off by the relative amount (the corruptions of the tests)."""
    n = len(rhs)
    L = np.zeros((n, n))
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            raise np.linalg.LinAlgError(f"pivot {j} not positive")
        L[j, j] = np.sqrt(d)
        r = (1.0 / L[j, j]) if rcp is None else rcp(L[j, j])
        if j == bad_pivot:
            r *= 1.0 + bad_rel
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) * r
    z = np.zeros(n)
    for i in range(n):
        z[i] = (rhs[i] - L[i, :i] @ z[:i]) / L[i, i]
    y = np.zeros(n)
    for i in range(n - 1, -1, -1):
        y[i] = (z[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def rcp_newton(x, steps):
    """1 / x from an estimate good to 2^-26 (the accuracy csrc/dev_math.h states for the hardware's) and `steps` Newton steps."""
    y = (1.0 / x) * (1.0 + 2.0 ** -26)
    for _ in range(steps):
        y = y + y * (1.0 - x * y)
    return y


# ------------------------------------------------------------------------------------------------------------------------
# the report on one computation and the bars
# ------------------------------------------------------------------------------------------------------------------------
def _rel_entries(got, hp):
    """worst per-entry relative deviation in units of eps; an entry that is zero in 50 digits must be zero (inf otherwise)."""
    worst = 0.0
    for x, h in zip(np.asarray(got, float).reshape(-1), np.asarray(hp, dtype=object).reshape(-1)):
        d = abs(mp.mpf(float(x)) - h)
        if h != 0:
            worst = max(worst, float(d / abs(h)) / EPS)
        elif d != 0:
            worst = np.inf
    return worst


def _rel(x, h):
    return float(abs(mp.mpf(float(x)) - h) / abs(h)) if h != 0 else (0.0 if x == 0 else np.inf)


class Reference:
    """The 50-digit side of one (inputs, mu): the reduced system of these very inputs, its certified solution, the model scalars."""

    def __init__(self, H, g, C, z1, mu, active, sch):
        H = np.asarray(H, dtype=object)
        if not isinstance(H[0, 0], mp.mpf):
            H = to_mp(H)
        self.H, self.g, self.mu, self.sch = H, g, mu, sch
        self.red = reduced_hp(H, g, C, z1, mu, active)
        self.Hd, self.gd, self.Cd, self.z1d = to_f(H), to_f(g), to_f(C), to_f(z1)
        self.Sd, self.rhs_d = to_f(self.red["S"]), to_f(self.red["rhs"])
        self.kappa = kappa2(self.Sd)
        self.y, self.cert, self.steps = solve_hp(self.red["S"], self.red["rhs"])
        self.model = model_hp(H, g, self.red, self.y, sch)
        self.normS, self.norm_rhs = float(np.linalg.norm(self.Sd)), float(mp.sqrt(_dot(self.red["rhs"], self.red["rhs"])))
        self.norm_y = float(mp.sqrt(_dot(self.y, self.y)))
        self.S_ld = self.Sd.astype(np.longdouble) + to_f(self.red["S"] - to_mp(self.Sd)).astype(np.longdouble)

    def report(self, out):
        """out: scale_p, diag_p, grad_p, gn_p, uc_grad (73), alpha and the q's by name — a device pass or a comparator.
        The residual of a double y is S (y - y_hp) (+ the certified residual of y_hp, below 1e-40): y - y_hp is formed in 50 digits and
        the product in extended precision, whose error 1e-19 |S| |y - y_hp| is at most kappa 1e-19 of the result."""
        red, m = self.red, self.model
        y = -(to_mp(out["gn_p"]) / to_mp(out["diag_p"]))
        dy = y - self.y
        dyf = to_f(dy).astype(np.longdouble)
        ny = float(np.linalg.norm(to_f(y)))
        rep = dict(kappa=self.kappa,
                   eta=float(np.linalg.norm(self.S_ld @ dyf)) / (self.normS * ny + self.norm_rhs) / EPS,
                   fwd=float(np.linalg.norm(dyf)) / self.norm_y / (EPS * self.kappa),
                   scale=_rel_entries(out["scale_p"], red["scale"]), diag=_rel_entries(out["diag_p"], red["diag"]),
                   grad=_rel_entries(out["grad_p"], red["grad"]), uc_grad=_rel_entries(out["uc_grad"][:KC], m["G"][:KC]),
                   alpha=_rel(out["alpha"], m["alpha"]) / (EPS * self.kappa))
        for k in Q_NAMES:
            rep[k] = _rel(out[k], m[k]) / (EPS if k in Q_WITHOUT_Y else EPS * self.kappa)
        return rep


def comparator_outputs(ref, y):
    """A double-precision solver's y (of ref.Sd, ref.rhs_d) through the device's interface: y after the round trip through
    gauss_newton_step_; scale, diagonal_, gradient_ and the scalars as a plain numpy evaluation in double."""
    rd = reduced_double(ref.Hd, ref.gd, ref.Cd, ref.z1d, ref.mu, ref.red["active"])
    gn = -(rd["diag"] * np.asarray(y, float))
    md = model_double(ref.Hd, ref.gd, rd, -gn / rd["diag"], ref.sch)
    out = dict(scale_p=rd["scale"], diag_p=rd["diag"], grad_p=rd["grad"], gn_p=gn, uc_grad=md["G"][:KC], alpha=md["alpha"])
    out.update({k: md[k] for k in Q_NAMES})
    return out


STEP_METRICS = ("eta", "fwd", "scale", "diag", "grad", "uc_grad", "alpha") + Q_NAMES
SCHUR_METRICS = ("C", "z1", "z2", "ls1", "ls2")
MARGIN = 16.0

# Worst value of each metric over the three comparators (LAPACK, the textbook loops, the oracle's schur_solve) and, for the Schur sums,
# over the two numpy orders, per case class of tests/test_solve_hp.py: as the CPU tests print them.  A bar is MARGIN x this.  Never a
# device figure.  The class of a case is (group, mu): the unit eps kappa_2(S) of the forward metrics moves with mu by orders of
# magnitude while the comparators' deviations in those metrics do not, so a worst value taken across mu would be set by the best
# conditioned system and mean nothing for the others.
COMPARATOR_WORST = {('regular', 1e-08): {'eta': 0.621,
                      'fwd': 0.911,
                      'scale': 1.66,
                      'diag': 2.11,
                      'grad': 2.45,
                      'uc_grad': 3.71,
                      'alpha': 1.1e-08,
                      'Q_GG': 4.32,
                      'Q_GN': 2.06e-08,
                      'Q_NN': 4.61e-08,
                      'Q_gG': 1.93,
                      'Q_gN': 1.06e-08,
                      'Q_GRAD_SQ': 1.68,
                      'Q_GN_SQ': 0.199,
                      'Q_GRAD_GN': 1.06e-08,
                      'C': 9.83,
                      'z1': 3.45,
                      'z2': 4.25,
                      'ls1': 7.6,
                      'ls2': 7.6},
 ('regular', 1e-05): {'eta': 0.482,
                      'fwd': 0.932,
                      'scale': 1.66,
                      'diag': 2.11,
                      'grad': 2.44,
                      'uc_grad': 3.71,
                      'alpha': 1.1e-05,
                      'Q_GG': 4.32,
                      'Q_GN': 1.02e-05,
                      'Q_NN': 2.04e-05,
                      'Q_gG': 1.93,
                      'Q_gN': 1.49e-05,
                      'Q_GRAD_SQ': 1.68,
                      'Q_GN_SQ': 0.00172,
                      'Q_GRAD_GN': 1.49e-05,
                      'C': 5.03,
                      'z1': 2.61,
                      'z2': 3.63,
                      'ls1': 4.72,
                      'ls2': 3.23},
 ('regular', 0.01): {'eta': 0.658,
                     'fwd': 1.29,
                     'scale': 1.66,
                     'diag': 2.11,
                     'grad': 2.44,
                     'uc_grad': 3.71,
                     'alpha': 0.0109,
                     'Q_GG': 4.32,
                     'Q_GN': 0.0153,
                     'Q_NN': 0.0294,
                     'Q_gG': 1.93,
                     'Q_gN': 0.0164,
                     'Q_GRAD_SQ': 1.68,
                     'Q_GN_SQ': 0.148,
                     'Q_GRAD_GN': 0.0131,
                     'C': 5.75,
                     'z1': 3.26,
                     'z2': 3.63,
                     'ls1': 4.72,
                     'ls2': 3.23},
 ('regular', 0.5): {'eta': 0.646,
                    'fwd': 2.54,
                    'scale': 1.66,
                    'diag': 2.11,
                    'grad': 2.44,
                    'uc_grad': 3.71,
                    'alpha': 0.477,
                    'Q_GG': 4.32,
                    'Q_GN': 0.613,
                    'Q_NN': 0.801,
                    'Q_gG': 1.93,
                    'Q_gN': 0.594,
                    'Q_GRAD_SQ': 1.68,
                    'Q_GN_SQ': 1.13,
                    'Q_GRAD_GN': 0.492,
                    'C': 6.25,
                    'z1': 3.1,
                    'z2': 3.63,
                    'ls1': 4.72,
                    'ls2': 3.23},
 ('weak', 1e-08): {'eta': 0.299,
                   'fwd': 0.00312,
                   'scale': 1.41,
                   'diag': 2.0,
                   'grad': 2.15,
                   'uc_grad': 3.59,
                   'alpha': 5.66e-11,
                   'Q_GG': 2.66,
                   'Q_GN': 0.000904,
                   'Q_NN': 0.00164,
                   'Q_gG': 0.784,
                   'Q_gN': 0.00105,
                   'Q_GRAD_SQ': 0.784,
                   'Q_GN_SQ': 0.00231,
                   'Q_GRAD_GN': 0.00105,
                   'C': 4.29,
                   'z1': 2.31,
                   'z2': 2.85,
                   'ls1': 0.893,
                   'ls2': 3.23},
 ('prior', 1e-08): {'eta': 0.213,
                    'fwd': 0.296,
                    'scale': 1.37,
                    'diag': 2.03,
                    'grad': 1.77,
                    'uc_grad': 3.25,
                    'alpha': 8.35e-10,
                    'Q_GG': 0.641,
                    'Q_GN': 0.05,
                    'Q_NN': 0.0732,
                    'Q_gG': 0.164,
                    'Q_gN': 0.0439,
                    'Q_GRAD_SQ': 0.164,
                    'Q_GN_SQ': 0.077,
                    'Q_GRAD_GN': 0.0439,
                    'C': 6.07,
                    'z1': 3.05,
                    'z2': 3.01,
                    'ls1': 1.49,
                    'ls2': 2.78},
 ('prior', 1e-05): {'eta': 0.313,
                    'fwd': 0.403,
                    'scale': 1.37,
                    'diag': 2.03,
                    'grad': 1.77,
                    'uc_grad': 3.25,
                    'alpha': 8.35e-07,
                    'Q_GG': 0.641,
                    'Q_GN': 0.00825,
                    'Q_NN': 0.00337,
                    'Q_gG': 0.164,
                    'Q_gN': 0.0103,
                    'Q_GRAD_SQ': 0.164,
                    'Q_GN_SQ': 0.194,
                    'Q_GRAD_GN': 0.0103,
                    'C': 6.16,
                    'z1': 2.85,
                    'z2': 3.01,
                    'ls1': 1.49,
                    'ls2': 2.78},
 ('prior', 0.01): {'eta': 0.59,
                   'fwd': 1.72,
                   'scale': 1.37,
                   'diag': 2.03,
                   'grad': 1.77,
                   'uc_grad': 3.25,
                   'alpha': 0.000832,
                   'Q_GG': 0.641,
                   'Q_GN': 0.143,
                   'Q_NN': 0.382,
                   'Q_gG': 0.164,
                   'Q_gN': 0.456,
                   'Q_GRAD_SQ': 0.164,
                   'Q_GN_SQ': 2.92,
                   'Q_GRAD_GN': 0.456,
                   'C': 5.47,
                   'z1': 2.59,
                   'z2': 3.01,
                   'ls1': 1.49,
                   'ls2': 2.78},
 ('prior', 0.5): {'eta': 0.282,
                  'fwd': 0.782,
                  'scale': 1.37,
                  'diag': 2.03,
                  'grad': 1.77,
                  'uc_grad': 3.25,
                  'alpha': 0.0309,
                  'Q_GG': 0.641,
                  'Q_GN': 0.817,
                  'Q_NN': 0.771,
                  'Q_gG': 0.164,
                  'Q_gN': 0.626,
                  'Q_GRAD_SQ': 0.164,
                  'Q_GN_SQ': 0.875,
                  'Q_GRAD_GN': 0.626,
                  'C': 6.06,
                  'z1': 1.98,
                  'z2': 3.01,
                  'ls1': 1.49,
                  'ls2': 2.78}}


# The metrics that involve neither y nor mu's effect on the conditioning — all in units of eps — are pooled over the classes: for
# them the three comparators are ONE numpy evaluation (the same at every mu of a case), so a class of one case would rest its bar on a
# single sample (the prior class: |gradient_|^2 within 0.16 eps by luck, where a sum of squares of entries good to 2.4 eps is not).
POOLED = ("scale", "diag", "grad", "uc_grad", "Q_GG", "Q_gG", "Q_GRAD_SQ") + SCHUR_METRICS
COMPARATOR_WORST["all"] = {m: max(d[m] for d in COMPARATOR_WORST.values()) for m in POOLED}


def bar(metric, cls):
    return MARGIN * COMPARATOR_WORST["all" if metric in POOLED else cls][metric]


def failed_checks(rep, metrics, cls):
    return [(k, rep[k], bar(k, cls)) for k in metrics if not rep[k] <= bar(k, cls)]
