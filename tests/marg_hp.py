"""50-digit and extended-precision checkers of the marginalization's linear algebra (test infrastructure: mpmath and numpy).

Two stages, as k_marg_solve (csrc/kernels_marg.h) has them:

  stage 1   A' = A_rr - A_rm A_mm^+ A_mr, b' = b_rr - A_rm A_mm^+ b_mm            schur_hp() states it in 50 digits
  stage 2   A' = V S V^T  ->  J0 = sqrt(S) V^T, r0 = V^T b' / sqrt(S), S > eps     factor_report() judges ONE computation's own
                                                                                   A', b', J0, r0 against a 50-digit spectrum

Every input double is taken exactly; results are rounded to double once.  The bars at the end of the file are 8 x the worst value
that two references (the oracle's eigen-solver and LAPACK's eigh, both in double) show over the case list of
tests/test_marg_hp.py — measured on the CPU, never against the kernel.
"""
import mpmath as mp
import numpy as np

from lfvio import abi

import marg_ref

DPS = 50
mp.mp.dps = DPS
EPS = marg_ref.EPS
U = 2.0 ** -52
LD = np.longdouble


def _f(x):
    return mp.mpf(float(x))


def marg_columns(kept_blocks, flag):
    """(dropped, kept) tangent columns of the 172-column layout for a prior's block list [(kind, shifted frame, idx)]."""
    if flag == abi.MARGIN_OLD:
        drop = marg_ref.tangent_cols(abi.BLOCK_POSE, 0) + marg_ref.tangent_cols(abi.BLOCK_SPEEDBIAS, 0)
    else:
        drop = marg_ref.tangent_cols(abi.BLOCK_POSE, abi.WINDOW_SIZE - 1)
    keep = []
    for kind, frame, idx in kept_blocks:
        assert idx == len(keep)
        if flag == abi.MARGIN_OLD and kind in (abi.BLOCK_POSE, abi.BLOCK_SPEEDBIAS):
            frame += 1  # undo addr_shift (estimator.cpp:921-933); MARGIN_SECOND_NEW shifts frame 10 only, which no prior holds
        keep += marg_ref.tangent_cols(kind, frame)
    return drop, keep


def prior_subwindow(w):
    """The factors of the MARGIN_SECOND_NEW marginalization as a window: the prior alone (estimator.cpp:942-966) — no landmark,
    every IMU factor switched off."""
    imu = []
    for p in w.imu:
        q = abi.preint_from_array(abi.preint_to_array(p))
        q.sum_dt = 1e9
        imu.append(q)
    return w.copy(start_frame=np.zeros(0, np.int32), obs_offset=np.zeros(1, np.int32), inv_depth=np.zeros(0), obs_point=np.zeros((0, 3)),
                  obs_velocity=np.zeros((0, 3)), obs_cur_td=np.zeros(0), obs_uv_y=np.zeros(0), imu=imu)


def marg_subwindow(w, flag):
    """The window whose linearization holds the sums of the marginalization's factors.  The extrinsic's columns are switched on:
    ResidualBlockInfo::Evaluate asks for every Jacobian, also of a block the solve holds constant (marginalization_factor.cpp:3-69)."""
    sub = marg_ref.frame0_subwindow(w) if flag == abi.MARGIN_OLD else prior_subwindow(w)
    return sub.copy(estimate_extrinsic=1)


def schur_hp(lin, kept_blocks, flag=abi.MARGIN_OLD):
    """The 50-digit statement of marg_ref.structured_marg_old, for both flags.  lin: a linearization (H, g, a, b, W) of
    marg_subwindow(post-gauge window, flag).  Landmarks are eliminated entry-wise where a > eps, the dropped block (pose 0 and
    speed/bias 0, 15 x 15, for MARGIN_OLD; pose 9 for MARGIN_SECOND_NEW) is pseudo-inverted through mp.eigsy with the eps cut.
    Returns a dict: A (n x n), b (n) rounded once; normH = ||H||_2 of the gathered system (dropped, kept and landmark columns, in
    double); lam_drop, the eigenvalues of the dropped block; b_scale, the denominator of the stage-1 bar of b' (see STAGE1_B)."""
    drop, keep = marg_columns(kept_blocks, flag)
    sel = drop + keep
    nd, nk, D = len(drop), len(keep), len(drop) + len(keep)
    Hd, gd = np.asarray(lin["H"], dtype=np.float64), np.asarray(lin["g"], dtype=np.float64)
    H = [[_f(Hd[r, c]) for c in sel] for r in sel]
    g = [_f(gd[c]) for c in sel]
    a, bl, W = lin["a"], lin["b"], lin["W"]
    where = {c: i for i, c in enumerate(sel) if c < abi.KC}
    used = []
    for l in range(len(a)):
        if not a[l] > EPS:
            continue
        used.append(l)
        inv = 1 / _f(a[l])
        nz = [(where[c], _f(W[l, c])) for c in np.flatnonzero(W[l]) if c in where]
        bi = _f(bl[l]) * inv
        for i, wi in nz:
            wia = wi * inv
            Hi = H[i]
            for j, wj in nz:
                Hi[j] -= wia * wj
            g[i] -= wi * bi
    # ||H||_2 of what was gathered: [[H_sel, W_sel^T], [W_sel, diag(a)]] over the landmarks that were eliminated
    Wk = np.zeros((len(used), D))
    for i, c in enumerate(sel):
        if c < abi.KC and len(used):
            Wk[:, i] = W[used, c]
    G = np.zeros((D + len(used), D + len(used)))
    G[:D, :D] = Hd[np.ix_(sel, sel)]
    G[D:, :D], G[:D, D:] = Wk, Wk.T
    G[D:, D:] = np.diag(np.asarray(a)[used])
    normH = float(np.linalg.norm(G, 2)) if G.size else 0.0
    out = dict(normH=normH, drop=drop, keep=keep)
    if nd == 0 or nk == 0:
        out.update(A=np.array([[float(H[nd + i][nd + j]) for j in range(nk)] for i in range(nk)]).reshape(nk, nk),
                   b=np.array([float(g[nd + i]) for i in range(nk)]), lam_drop=np.zeros(0), b_scale=1.0)
        return out
    Amm = mp.matrix(nd, nd)
    for i in range(nd):
        for j in range(nd):
            Amm[i, j] = (H[i][j] + H[j][i]) / 2
    E, Q = mp.eigsy(Amm)
    Ainv = [[mp.mpf(0)] * nd for _ in range(nd)]
    for k in range(nd):
        if E[k] > EPS:
            ie = 1 / E[k]
            for i in range(nd):
                qi = Q[i, k] * ie
                for j in range(nd):
                    Ainv[i][j] += qi * Q[j, k]
    T = [[mp.fsum(H[nd + i][k] * Ainv[k][j] for k in range(nd)) for j in range(nd)] for i in range(nk)]
    A = np.array([[float(H[nd + i][nd + j] - mp.fsum(T[i][k] * H[k][nd + j] for k in range(nd))) for j in range(nk)] for i in range(nk)])
    b = np.array([float(g[nd + i] - mp.fsum(T[i][k] * g[k] for k in range(nd))) for i in range(nk)])
    # the solution of the dropped block, x_m = A_mm^+ b_mm: b' = b_rr - A_rm x_m, and the rounding of the products A_rm x_m is
    # relative to ||A_rm|| ||x_m|| <= ||H||_2 ||x_m||_2
    xm = [mp.fsum(Ainv[i][k] * g[k] for k in range(nd)) for i in range(nd)]
    norm_xm = float(mp.sqrt(mp.fsum(x * x for x in xm)))
    out.update(A=A, b=b, lam_drop=np.array(sorted(float(x) for x in E)), b_scale=normH * norm_xm)
    return out


def stage1_report(A, b, hp):
    """One computation's A', b' against schur_hp's: dA = ||A' - A'_hp||_2 in units of u ||H||_2 and db = max|b' - b'_hp| in
    units of u STAGE1_B, STAGE1_B = ||H||_2 ||A_mm^+ b_mm||_2 (the size of the products A_rm x_m that b' is the remainder of)."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if A.size == 0:
        return dict(dA=0.0, db=0.0)
    return dict(dA=float(np.linalg.norm(A - hp["A"], 2) / (U * hp["normH"])), db=float(np.abs(b - hp["b"]).max() / (U * hp["b_scale"])))


def eigvals_hp(A):
    """The eigenvalues of (A + A^T) / 2 from a 50-digit solve, ascending, rounded to double once."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    if n == 0:
        return np.zeros(0)
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = (_f(A[i, j]) + _f(A[j, i])) / 2
    E = mp.eigsy(M, eigvals_only=True)
    return np.array(sorted(float(x) for x in E))


def factor_report(A, b, J, r, lam_hp=None, ev_bar=None):
    """Judge ONE computation's own A', b', J0, r0 (marginalization_factor.cpp:283-291).  Products are formed in np.longdouble
    (2^-64: the checker's own rounding is 2^-11 of the bars).  A row is a KEPT row when ||J_i||^2 > eps / 2: the solvers keep
    S > eps and write J_i = sqrt(S) v_i with ||v_i||^2 = 1 to a few u, so a kept row's squared norm is S (1 +- 1e-14) — and whatever
    else lies in a row that is not kept is held against exact zero.  Returns, in units of u ||A'||_2 unless noted:

      ev       max |sort(S_kept) - lam_hp[top k]|,  S_i = ||J_i||^2, k = the number of kept rows
      cut_ok   every lam_hp > eps + band is kept and every lam_hp < eps - band is dropped, band = ev_bar u ||A'||_2: the count k
               gets no other slack.  (marg_ref.kept_count_slack, which check_prior uses, allows for the rounding of A' between two
               computations — 1e4 times as much; this rule is the sharper one: it judges the count on the computation's own A'.)
               cut_need is the smallest band (same units) under which k would pass, in_band the eigenvalues within the band
      res      max_i ||A' v_i - S_i v_i||_2,  v_i = J_i / sqrt(S_i)
      recon    ||J^T J - A'||_2 - max_dropped |lam_hp|: a direction lost to parallel vectors inside the kept spectrum shows here
      r        max_i |r_i - v_i . b' / sqrt(S_i)| / (sum_k |v_ik b'_k| / sqrt(S_i)),  in units of u
      exact    zero_rows (rows that are not kept are exactly zero in J0 and r0), dropped_first, ascending (kept S), finite
    """
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    ev_bar = BAR_EV if ev_bar is None else ev_bar
    finite = bool(np.all(np.isfinite(J)) and np.all(np.isfinite(r)) and np.all(np.isfinite(A)) and np.all(np.isfinite(b)))
    if n == 0:
        return dict(n=0, k=0, normA=0.0, ev=0.0, res=0.0, recon=0.0, r=0.0, cut_ok=True, cut_need=0.0, in_band=0,
                    exact=dict(zero_rows=True, dropped_first=True, ascending=True, finite=finite))
    lam = eigvals_hp(A) if lam_hp is None else np.asarray(lam_hp)
    normA = float(np.abs(lam).max())
    unit = U * normA
    Al = 0.5 * (A.astype(LD) + A.T.astype(LD))
    Jl, rl, bl = np.asarray(J).astype(LD), np.asarray(r).astype(LD), np.asarray(b).astype(LD)
    S = (Jl * Jl).sum(axis=1)
    kept = S > LD(EPS) / 2
    k = int(kept.sum())
    idx = np.flatnonzero(kept)
    exact = dict(zero_rows=bool(np.all(np.asarray(J)[~kept] == 0.0) and np.all(np.asarray(r)[~kept] == 0.0)),
                 dropped_first=bool(k == 0 or idx[0] == n - k),
                 ascending=bool(np.all(np.diff(S[kept]) >= 0)), finite=finite)
    band = ev_bar * unit
    lo, hi = int((lam > EPS + band).sum()), int((lam >= EPS - band).sum())
    # the band k itself would need: its smallest kept eigenvalue must not lie below eps - band, its largest dropped one not above eps + band
    need = max(0.0, EPS - lam[n - k] if k > 0 else 0.0, lam[n - k - 1] - EPS if k < n else 0.0)
    out = dict(n=n, k=k, normA=normA, cut_ok=bool(lo <= k <= hi), cut_need=float(need / unit), in_band=hi - lo, exact=exact,
               ev=0.0, res=0.0, r=0.0, lam=lam)
    lam_dropped = float(np.abs(lam[: n - k]).max()) if k < n else 0.0
    out["recon"] = float((np.linalg.norm((Jl.T @ Jl - Al).astype(np.float64), 2) - lam_dropped) / unit)
    if k:
        Sk = S[kept]
        rt = np.sqrt(Sk)
        V = Jl[kept] / rt[:, None]
        out["ev"] = float(np.abs(np.sort(Sk) - lam[n - k:].astype(LD)).max() / unit)
        R = Al @ V.T - V.T * Sk[None, :]
        out["res"] = float(np.sqrt((R * R).sum(axis=0)).max() / unit)
        num = np.abs(rl[kept] - (V @ bl) / rt)
        den = (np.abs(V) @ np.abs(bl)) / rt
        out["r"] = float((num / np.where(den > 0, den, LD(1))).max() / U)
    return out


def lapack_factor(A, b):
    """The reference's second half with LAPACK's eigh: J0, r0 of A', b' (rows ascending, the dropped ones zero)."""
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = lam > EPS
    J = np.where(keep[:, None], np.sqrt(np.where(keep, lam, 0.0))[:, None] * V.T, 0.0)
    r = np.where(keep, (V.T @ b) / np.sqrt(np.where(keep, lam, 1.0)), 0.0)
    return J, r


def failed_checks(rep, s1=None):
    """The names of the checks a report misses, against the bars below."""
    bad = [k for k, bar in (("ev", BAR_EV), ("res", BAR_RES), ("recon", BAR_RECON), ("r", BAR_R)) if not rep[k] <= bar]
    if not rep["cut_ok"]:
        bad.append("cut_ok")
    bad += [k for k, ok in rep["exact"].items() if not ok]
    if s1 is not None:
        bad += [k for k, bar in (("dA", BAR_STAGE1_A), ("db", BAR_STAGE1_B)) if not s1[k] <= bar]
    return sorted(bad)


# ---- the bars: 8 x the worst value of two double references over the case list of tests/test_marg_hp.py (21 variants: n = 15 ... 76,
# ||A'||_2 = 2e-5 ... 4e6, ||H||_2 = 2e5 ... 2.4e10).  Stage 2: (the oracle's eigen-solver, LAPACK's eigh) on the oracle's A', b'.
# Stage 1: (the oracle's dense A', b', numpy's structured statement) against schur_hp.  Three bits of room for other error constants
# and other orders of summation; measured on the CPU, never against the kernel.
REF_EV, REF_RES, REF_RECON, REF_R = (24.11, 16.91), (24.32, 17.08), (17.32, 9.48), (19.40, 9.56)
REF_STAGE1_A, REF_STAGE1_B = (12.91, 69.54), (3.36, 2.28)
BAR_EV = 8 * max(REF_EV)            # 192.9 u ||A'||_2
BAR_RES = 8 * max(REF_RES)          # 194.6 u ||A'||_2
BAR_RECON = 8 * max(REF_RECON)      # 138.6 u ||A'||_2
BAR_R = 8 * max(REF_R)              # 155.2 u
BAR_STAGE1_A = 8 * max(REF_STAGE1_A)  # 556.3 u ||H||_2 (the structured statement on cut_n40, whose 6 x 6 dropped block is ill-conditioned; 12.9 elsewhere)
# STAGE1_B, the denominator of b': ||H||_2 ||A_mm^+ b_mm||_2.  Under it the two references' worst values are 3.4 and 2.3 u and every case
# lies within 0.004 ... 3.4; under the sum of the magnitudes that enter b' (|b_rr| + |A_rm A_mm^+| |b_mm|, landmark terms included) they
# spread over 0.06 ... 565.
BAR_STAGE1_B = 8 * max(REF_STAGE1_B)  # 26.9 u ||H||_2 ||x_m||_2
