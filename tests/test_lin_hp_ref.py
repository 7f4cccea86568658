"""CPU tests of the 50-digit statement of the linearization (tests/lin_hp.py) and of the bars tests/test_lin_hp.py holds the device to.

a. The statement's Jacobians against central differences of its own residuals in 50 digits (h = 1e-20): what makes the statement
   independent of the memory of Ceres and of the reference's formulas that np_ref.py and oracle/ share.  Quaternions are normalized in
   50 digits first (the analytic forms are derivatives on the unit sphere; a double quaternion is off it by 1e-16).  Three blocks of the
   reference are NOT derivatives, and are held by their formula instead:
     * the td column of the visual factor (projection_td_factor.cpp:143-144; np_ref.TD_TRUE_DERIVATIVE names the difference): the
       true-derivative form is differenced, the coded form is that minus sqrt_info (B N(pj) velocity_j - velocity_j.head(2));
     * the rotation rows of the IMU factor against theta_i (imu_factor.h:100): (1 + |dq_dbg dbg|^2 / 4) x the derivative — deltaQ leaves
       corrected_delta_q off the unit sphere by that factor, the residual divides by it, the coded block multiplies;
     * the rotation rows against bg_i (imu_factor.h:132): the derivative at dbg = 0, and within 4 |dq_dbg dbg| of it elsewhere;
     * the prior's Jacobian (marginalization_factor.cpp:376): J0 itself, which is the derivative where the state is x0; elsewhere the
       derivative is J0 diag(I, [Qleft(dq)]_br) per pose block, which is what is differenced.
b. The comparators (np_ref.assemble, oracle.linearize and their factors) against the statement on every case of tests/lin_cases.py, per
   metric and class: lin_hp.COMPARATOR_WORST is their worst, and a test asserts that the table reproduces.  The comparators' own last
   bits move with the BLAS kernel numpy picks for a CPU (np_ref multiplies its 3 x 3 matrices with `@`), so "reproduces" is: no figure
   above 1.5 x the table's, none below a third of it.  The device's bars are 16 x the table, whatever a machine measures.
c. Planted errors, each applied to a copy of a comparator's output: it passes test_gpu_parity.check_linearization against the unspoilt
   result and fails the new checks (the metric that catches it is printed).  1e-9 in one entry of an (ex, pose_j) block, of the td
   entry of one landmark's W and of a pose-pose block of frames that are not neighbours do so on ordinary windows (n33, prior_old).  One
   observation left out, one landmark weighted at s = 0 and the td column as the true derivative change that landmark's a, b, W by
   1e-3 .. 1 of the arrays' largest entries on an ordinary window, where the flat check sees them; it is blind to them where one
   landmark dominates every array (close_point below), and there they are planted.
d. Preconditions per case: the certificate (the 50-digit result unchanged at 80 digits to 1e-40), every metric finite for both
   comparators (no case, no block and no landmark left out: the share excluded is zero), the corrector's alpha branch never taken.
"""
import mpmath as mp
import numpy as np
import pytest

from lfvio import abi, synth

import lin_cases as lc
import lin_hp as lh
import np_ref
from test_gpu_parity import check_linearization

REPRODUCE_ABOVE, REPRODUCE_BELOW = 1.5, 3.0

statement, comparator_reports = lc.statement, lc.comparator_reports


# ------------------------------------------------------------------------------------------------------------------------
# a. finite differences
# ------------------------------------------------------------------------------------------------------------------------
H_FD = mp.mpf(10) ** -20
FD_TOL = 1e-27  # rounding 1e-50 / h = 1e-30 of the residual's terms, times what the chain amplifies (measured: 1e-31 .. 1e-29)


def _unit_pose(p):
    q = p[3:7]
    n = lh._norm(q)
    out = p.copy()
    out[3:7] = q / n
    return out


def _plus_pose(p, d):
    """pose_local_parameterization.cpp:3-27: p + dp, (q * deltaQ(dtheta)).normalized(); quaternion stored x y z w."""
    q = lh._qmul(lh._pose_q(p), lh._deltaQ(d[3:6]))
    q = q / lh._norm(q)
    out = p.copy()
    out[:3] = p[:3] + d[:3]
    out[3:7] = [q[1], q[2], q[3], q[0]]
    return out


def _central(fun, n):
    """columns (f(+h e_k) - f(-h e_k)) / 2h"""
    cols = []
    for k in range(n):
        d = lh._zeros(n)
        d[k] = H_FD
        cols.append((fun(d) - fun(-d)) / (2 * H_FD))
    return np.stack(cols, axis=1)


def _rel(A, B):
    A, B = np.asarray(A, dtype=object), np.asarray(B, dtype=object)
    scale = max(abs(v) for v in B.ravel())
    return float(max(abs(a - b) for a, b in zip(A.ravel(), B.ravel())) / scale) if scale != 0 else float(max(abs(a) for a in A.ravel()))


FD_WINDOWS = {"n7": lambda: synth.make_window(3, 7), "ocam_rs": lambda: synth.make_window(6, 5, camera="ocam", tr=0.02)}


@pytest.mark.parametrize("name", list(FD_WINDOWS))
def test_visual_jacobians_are_the_derivatives_of_the_residual(name):
    w = FD_WINDOWS[name]()
    st, obs = lh.State(w), lh.obs_mp(w)
    st.pose = np.stack([_unit_pose(p) for p in st.pose])
    st.ex = _unit_pose(st.ex)
    worst = dict(pose_i=0.0, pose_j=0.0, ex=0.0, td=0.0, lam=0.0, td_coded=0.0)
    for l, o0, o, fi, fj in lh.observations(w):
        args = (True, obs["TR"], obs["ROW"], obs["s"], obs["pt"][o0], obs["pt"][o], obs["vel"][o0], obs["vel"][o], obs["ctd"][o0], obs["ctd"][o],
                obs["uvy"][o0], obs["uvy"][o])
        r, J, *_ = lh.visual(*args, st.pose[fi], st.pose[fj], st.ex, st.lam[l], st.td, td_true=True)
        _, Jc, *_ = lh.visual(*args, st.pose[fi], st.pose[fj], st.ex, st.lam[l], st.td)
        res = lambda pi, pj, ex, lam, td: lh.visual(*args, pi, pj, ex, lam, td, want_J=False)[0]  # noqa: E731
        worst["pose_i"] = max(worst["pose_i"], _rel(_central(lambda d: res(_plus_pose(st.pose[fi], d), st.pose[fj], st.ex, st.lam[l], st.td), 6), J[:, 0:6]))
        worst["pose_j"] = max(worst["pose_j"], _rel(_central(lambda d: res(st.pose[fi], _plus_pose(st.pose[fj], d), st.ex, st.lam[l], st.td), 6), J[:, 6:12]))
        worst["ex"] = max(worst["ex"], _rel(_central(lambda d: res(st.pose[fi], st.pose[fj], _plus_pose(st.ex, d), st.lam[l], st.td), 6), J[:, 12:18]))
        worst["td"] = max(worst["td"], _rel(_central(lambda d: res(st.pose[fi], st.pose[fj], st.ex, st.lam[l], st.td + d[0]), 1), J[:, 18:19]))
        worst["lam"] = max(worst["lam"], _rel(_central(lambda d: res(st.pose[fi], st.pose[fj], st.ex, st.lam[l] + d[0], st.td), 1), J[:, 19:20]))
        # the coded td column by its formula: the second term is sqrt_info velocity_j.head(2) where the derivative has sqrt_info B N(pj) velocity_j
        B, _ = lh.tangent_base(obs["pt"][o])
        row_j = obs["uvy"][o] - obs["ROW"] / 2
        pj = obs["pt"][o] - (st.td - obs["ctd"][o] + obs["TR"] / obs["ROW"] * row_j) * obs["vel"][o]
        m = lh._norm(pj)
        true_second = obs["s"] * B.dot((lh._eye(3) / m - np.outer(pj, pj) / (m * m * m)).dot(obs["vel"][o]))
        worst["td_coded"] = max(worst["td_coded"], _rel(Jc[:, 18] - J[:, 18], obs["s"] * obs["vel"][o][:2] - true_second))
        assert _rel(Jc[:, :18], J[:, :18]) == 0.0 and _rel(Jc[:, 19], J[:, 19]) == 0.0
    print(name, "visual factors", w.M - w.N, {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < FD_TOL


@pytest.mark.parametrize("name", list(FD_WINDOWS))
def test_imu_jacobians_are_the_derivatives_of_the_residual(name):
    w = FD_WINDOWS[name]()
    st = lh.State(w)
    st.pose = np.stack([_unit_pose(p) for p in st.pose])
    G = lh.to_mp(np.asarray(w.g, float))
    worst = dict(fd=0.0, theta_i=0.0, bg_at_zero=0.0, bg_off=0.0)
    for f in range(10):
        fld = lh.pre_fields(w.imu[f])
        fld["dq"] = fld["dq"] / lh._norm(fld["dq"])
        pi, si, pj, sj = st.pose[f], st.sb[f], st.pose[f + 1], st.sb[f + 1]
        r, Je, *_ = lh.imu_raw(fld, G, pi, si, pj, sj, exact_rotation=True)
        _, Jc, *_ = lh.imu_raw(fld, G, pi, si, pj, sj)
        res = lambda a, b, c, d: lh.imu_raw(fld, G, a, b, c, d, want_J=False)[0]  # noqa: E731
        fd = np.hstack([_central(lambda d: res(_plus_pose(pi, d), si, pj, sj), 6), _central(lambda d: res(pi, si + d, pj, sj), 9),
                        _central(lambda d: res(pi, si, _plus_pose(pj, d), sj), 6), _central(lambda d: res(pi, si, pj, sj + d), 9)])
        for c0, c1 in ((0, 6), (6, 15), (15, 21), (21, 30)):
            worst["fd"] = max(worst["fd"], _rel(fd[:, c0:c1], Je[:, c0:c1]))
        # the coded forms: everything but two blocks is the derivative as it stands
        same = np.ones((15, 30), dtype=bool)
        same[3:6, 3:6] = same[3:6, 12:15] = False
        assert _rel(np.where(same, Jc, 0), np.where(same, Je, 0)) < 1e-45
        phi = fld["J"][3:6, 12:15].dot(si[6:9] - fld["bg"])
        rho2 = 1 + (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) / 4
        worst["theta_i"] = max(worst["theta_i"], _rel(Jc[3:6, 3:6], rho2 * Je[3:6, 3:6]))
        worst["bg_off"] = max(worst["bg_off"], _rel(Jc[3:6, 12:15], Je[3:6, 12:15]) / float(lh._norm(phi)))
        at0 = dict(fld, bg=si[6:9])
        worst["bg_at_zero"] = max(worst["bg_at_zero"], _rel(lh.imu_raw(at0, G, pi, si, pj, sj)[1][3:6, 12:15],
                                                             lh.imu_raw(at0, G, pi, si, pj, sj, exact_rotation=True)[1][3:6, 12:15]))
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    assert worst["fd"] < FD_TOL and worst["theta_i"] < 1e-45 and worst["bg_at_zero"] < 1e-45 and worst["bg_off"] < 4.0


def test_sqrt_info_is_the_transposed_cholesky_factor_of_the_inverse():
    w = synth.make_window(3, 7)
    P = lh.pre_fields(w.imu[2])["P"]
    S = lh.sqrt_info(P)
    assert all(S[i, j] == 0 for i in range(15) for j in range(i))  # upper triangular: matrixL().transpose()
    Pi = lh.inverse(P)
    assert _rel(Pi.dot(P), lh._eye(15)) < 1e-40                    # (kappa 1e4 of 50 digits)
    assert _rel(np.tril(S.T.dot(S)), np.tril(Pi)) < 1e-40          # S^T S = the lower triangle of P^-1, mirrored: what LLT reads
    assert np.abs(lh.to_f(S) - np_ref.imu(w.imu[2], w.g, w.pose[2], w.speed_bias[2], w.pose[3], w.speed_bias[3])[5]).max() < 1e-8 * np.abs(lh.to_f(S)).max()


def test_prior_jacobian_is_the_derivative_where_the_state_is_x0_and_its_chain_elsewhere(oracle):
    w = lc.window(oracle, "prior_old")
    pr = w.prior
    J0 = lh.to_mp(pr.J())
    r0 = lh.to_mp(pr.r())

    class S:
        def __init__(self, blocks):
            self.blocks = blocks

        def block(self, kind, frame):
            return self.blocks[(kind, frame)]

    st = lh.State(w)
    here = {(pr.blocks[i].kind, pr.blocks[i].frame): st.block(pr.blocks[i].kind, pr.blocks[i].frame) for i in range(pr.num_blocks)}
    here = {k: (_unit_pose(v) if k[0] in (0, 2) else v) for k, v in here.items()}
    at_x0 = {(pr.blocks[i].kind, pr.blocks[i].frame): lh.to_mp(np.array(pr.block_x0[i][:])) for i in range(pr.num_blocks)}
    at_x0 = {k: (_unit_pose(v) if k[0] in (0, 2) else v[:9 if k[0] == 1 else 1]) for k, v in at_x0.items()}
    worst = dict(at_x0=0.0, chain=0.0)
    for tag, base in (("at_x0", at_x0), ("chain", here)):
        for i in range(pr.num_blocks):
            key, idx = (pr.blocks[i].kind, pr.blocks[i].frame), pr.block_idx[i]
            ls = np_ref.block_local(key[0])

            def res(d):
                blocks = dict(base)
                blocks[key] = _plus_pose(base[key], d) if key[0] in (0, 2) else base[key] + d
                # x0 taken at its normalized quaternion too: the prior's own doubles are off the sphere by 1e-16
                dx = _dx(pr, S(blocks), at_x0)
                return r0 + J0.dot(dx)

            D = lh._eye(ls)
            if key[0] in (0, 2):
                dq = lh._qmul(lh._qinv(lh._pose_q(at_x0[key])), lh._pose_q(base[key]))
                D[3:6, 3:6] = lh._Qleft(dq)[1:, 1:] * (1 if dq[0] >= 0 else -1)
            worst[tag] = max(worst[tag], _rel(_central(res, ls), J0[:, idx:idx + ls].dot(D)))
    print("prior", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < FD_TOL


def _dx(pr, st, x0s):
    """lin_hp.prior_dx with x0 replaced by the given (normalized) one"""
    dx = lh._zeros(pr.n)
    for i in range(pr.num_blocks):
        kind, frame, idx = pr.blocks[i].kind, pr.blocks[i].frame, pr.block_idx[i]
        x, x0 = st.block(kind, frame), x0s[(kind, frame)]
        if kind in (0, 2):
            dx[idx:idx + 3] = x[:3] - x0[:3]
            dq = lh._qmul(lh._qinv(lh._pose_q(x0)), lh._pose_q(x))
            dx[idx + 3:idx + 6] = 2 * dq[1:] * (1 if dq[0] >= 0 else -1)
        else:
            sz = 9 if kind == 1 else 1
            dx[idx:idx + sz] = x[:sz] - x0[:sz]
    return dx


def test_prior_dx_is_the_references_and_takes_the_sign_branch(oracle):
    for name, flipped in (("prior_old", False), ("prior_negated", True)):
        w = lc.window(oracle, name)
        dx, fl = lh.prior_dx(w.prior, lh.State(w))
        assert bool(fl) == flipped, (name, fl)
        r, _ = np_ref.prior_eval(w.prior, np_ref.St(w))
        stm = statement(oracle, name)
        assert stm.prior_flipped == fl
        rr = w.prior.r() + w.prior.J() @ lh.to_f(dx)
        assert np.abs(rr - r).max() <= 1e-9 * np.abs(r).max()


def test_tangent_base_branch():
    one = lh.to_mp([0.0, 0.0, 1.0])
    B, br = lh.tangent_base(one)
    assert br and [float(v) for v in B.ravel()] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    B, br = lh.tangent_base(lh.to_mp(np.array([1e-9, 0.0, 1.0]) / np.linalg.norm([1e-9, 0.0, 1.0])))
    assert not br and abs(float(B[0, 0]) + 1.0) < 1e-15 and abs(float(B[0, 2]) - 1e-9) < 1e-20


# ------------------------------------------------------------------------------------------------------------------------
# b, d. the comparators on every case
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_preconditions_and_comparators(oracle, name):
    """The certificate; every metric of both comparators finite (nothing excluded) and inside 1.5 / 16 of its bar (the table is their
    worst: inside 1 / 16 by construction on the machine that measured it)."""
    w, stm = lc.window(oracle, name), statement(oracle, name)
    cert = lh.certificate(w, stm)
    reps = comparator_reports(oracle, name)
    cls = lc.case_class(name)
    for k, rep in reps.items():
        print(f"{name} [{cls}] {k}: " + " ".join(f"{m}={rep[m]:.3g}" for m in lh.ALL_METRICS))
    print(f"{name}: N={w.N} factors={stm.num_factors} certificate={cert:.1e} kappa(P)={stm.imu_kappa.max():.3g}")
    assert cert < lh.CERTIFICATE
    assert lh.ALPHA_TAKEN[0] == 0
    for k, rep in reps.items():
        assert set(rep) == set(lh.ALL_METRICS) and all(np.isfinite(rep[m]) for m in lh.ALL_METRICS), (k, rep)
        assert lh.failed_checks(rep, lh.ALL_METRICS, cls, margin=REPRODUCE_ABOVE) == [], k


def measured_table(oracle):
    table = {c: {m: 0.0 for m in lh.ALL_METRICS} for c in lc.CLASSES}
    for name in lc.NAMES:
        for rep in comparator_reports(oracle, name).values():
            for m in lh.ALL_METRICS:
                table[lc.case_class(name)][m] = max(table[lc.case_class(name)][m], rep[m])
    return table


def test_comparator_table_reproduces(oracle):
    table = measured_table(oracle)
    print("COMPARATOR_WORST = {")
    for c in lc.CLASSES:
        print(f"    {c!r}: {{" + ", ".join(f"{m!r}: {float(f'{table[c][m]:.3g}')!r}" for m in lh.ALL_METRICS) + "},")
    print("}")
    assert set(lh.COMPARATOR_WORST) == set(lc.CLASSES)
    for c in lc.CLASSES:
        for m in lh.ALL_METRICS:
            t, v = lh.COMPARATOR_WORST[c][m], table[c][m]
            assert v <= REPRODUCE_ABOVE * t and v * REPRODUCE_BELOW >= t, (c, m, t, v)
    # every class is populated and no case is left out of its class
    assert sorted(set(lc.case_class(n) for n in lc.NAMES)) == sorted(lc.CLASSES) and len(lc._rep) == len(lc.NAMES)


def test_case_list_covers_what_it_says(oracle):
    seen = set()
    for name in lc.NAMES:
        w = lc.window(oracle, name)
        seen |= set(zip(w.start_frame.tolist(), np.diff(w.obs_offset).tolist()))
    assert seen >= {(s, k) for s in range(10) for k in range(2, abi.NUM_FRAMES - s + 1)}
    assert [lc.window(oracle, n).N for n in ("n1", "n7", "n31", "n32", "n33", "n63", "n64", "n65", "n320", "n321")] == [1, 7, 31, 32, 33, 63, 64, 65, 320, 321]
    w = lc.window(oracle, "pair_chunks")
    pairs = np.zeros((11, 11), int)
    for l, o0, o, fi, fj in lh.observations(w):
        pairs[fi, fj] += 1
    assert sorted(pairs[pairs > 0].tolist()) == [1, 15, 16, 17, 63, 64, 65]
    assert (lc.window(oracle, "prior78").prior.n, lc.window(oracle, "prior90").prior.n) == (78, 90)
    assert lc.window(oracle, "prior_old").prior.n <= 76 and lc.window(oracle, "prior_second_new").prior.valid == 1
    assert lc.window(oracle, "imu_skip").imu[4].sum_dt == 10.5 and lc.window(oracle, "imu_keep10").imu[4].sum_dt == 10.0
    assert not statement(oracle, "imu_skip").imu_kept[4] and statement(oracle, "imu_keep10").imu_kept[4]
    w = lc.window(oracle, "zero_residual")
    r, *_ = lh.visual_of(w, lh.State(w), 0, 0, 1, 0, 1, lh.obs_mp(w), want_J=False)
    assert r[0] == 0 and r[1] == 0
    rr = np_ref.visual(False, w.tr, w.row, w.sqrt_info, w.obs_point[0], w.obs_point[1], w.obs_velocity[0], w.obs_velocity[1], 0.0, 0.0, 0.0, 0.0,
                       w.pose[0], w.pose[1], w.ex_pose, w.inv_depth[0], w.td)[0]
    assert rr[0] == 0.0 and rr[1] == 0.0
    w = lc.window(oracle, "displaced")
    s = [float(sum(x * x for x in lh.visual_of(w, lh.State(w), l, o0, o, fi, fj, lh.obs_mp(w), want_J=False)[0])) for l, o0, o, fi, fj in lh.observations(w)]
    assert 3e3 < max(s) < 3e4, max(s)
    w = lc.window(oracle, "on_axis")
    assert lh.tangent_base(lh.to_mp(w.obs_point[w.obs_offset[0] + 1]))[1] and not lh.tangent_base(lh.to_mp(w.obs_point[w.obs_offset[1] + 1]))[1]
    assert abs(np.linalg.norm(lc.window(oracle, "offs_frame10").pose[10, 3:]) - 1.0 - 1e-8) < 1e-10


# ------------------------------------------------------------------------------------------------------------------------
# c. planted errors
# ------------------------------------------------------------------------------------------------------------------------
def close_point(oracle):
    """A window in which one landmark lies 1e-12 m beside the centre of the second camera that sees it, and is seen there half a residual
    unit off: its Jacobians are 1e12 and more, and every array of the linearization (b through J_lambda r) has an entry many orders above
    the rest; an IMU factor kept at sum_dt = 10 puts 1e12 and more into the cost.  The flat 1e-10 of test_gpu_parity.check_linearization then sees nothing of any other landmark.  The close landmark's
    bearing velocities are zero, so its own td column is the same in the coded and in the true-derivative form."""
    w = lc.with_sum_dt(synth.make_window(5, 33), 4, 10.0).copy()
    l = int(np.nonzero(np.diff(w.obs_offset) == 2)[0][0])
    o0, fi = int(w.obs_offset[l]), int(w.start_frame[l])
    qi, qj, qe = np_ref.pose_q(w.pose[fi]), np_ref.pose_q(w.pose[fi + 1]), np_ref.pose_q(w.ex_pose)
    ci = np_ref.qrot(qi, w.ex_pose[:3]) + w.pose[fi, :3]
    cj = np_ref.qrot(qj, w.ex_pose[:3]) + w.pose[fi + 1, :3]
    side = np.cross(cj - ci, [0.2, 0.9, -0.4])
    X = cj + 1e-12 * side / np.linalg.norm(side)
    d = np_ref.qrot(np_ref.qinv(qe), np_ref.qrot(np_ref.qinv(qi), X - ci))  # the point in camera i
    w.obs_point[o0] = d / np.linalg.norm(d)
    w.inv_depth[l] = 1.0 / np.linalg.norm(d)
    Xb = np_ref.qrot(qe, w.obs_point[o0] / w.inv_depth[l]) + w.ex_pose[:3]
    Xcj = np_ref.qrot(np_ref.qinv(qe), np_ref.qrot(np_ref.qinv(qj), np_ref.qrot(qi, Xb) + w.pose[fi, :3] - w.pose[fi + 1, :3]) - w.ex_pose[:3])
    u = Xcj / np.linalg.norm(Xcj)
    t = np.cross(u, [0.5, 0.1, 0.7])
    w.obs_point[o0 + 1] = u + 0.005 * t / np.linalg.norm(t)
    w.obs_velocity[o0:o0 + 2] = 0.0
    return w, l


def landmark_terms(w, l, weighted):
    """The contribution of landmark l's factors to (H, g, a_l, b_l, W_l, cost) from np_ref's factors, with the Cauchy weight or at s = 0."""
    st = np_ref.St(w)
    H, g, W, a, b, cost = np.zeros((lh.KP, lh.KP)), np.zeros(lh.KP), np.zeros(lh.KC), 0.0, 0.0, 0.0
    o0, fi = int(w.obs_offset[l]), int(w.start_frame[l])
    for o in range(o0 + 1, int(w.obs_offset[l + 1])):
        fj = fi + o - o0
        r, Ji, Jj, Jex, Jl, Jtd = np_ref.visual(bool(w.estimate_td), w.tr, w.row, w.sqrt_info, w.obs_point[o0], w.obs_point[o], w.obs_velocity[o0],
                                                w.obs_velocity[o], w.obs_cur_td[o0], w.obs_cur_td[o], w.obs_uv_y[o0], w.obs_uv_y[o], st.pose[fi],
                                                st.pose[fj], st.ex, st.lam[l], st.td)
        J = np.zeros((2, lh.KC + 1))
        J[:, 6 * fi:6 * fi + 6], J[:, 6 * fj:6 * fj + 6], J[:, 66:72], J[:, 72], J[:, 73] = Ji[:, :6], Jj[:, :6], Jex[:, :6], Jtd, Jl
        if weighted:
            rho0, r, J = np_ref.cauchy_correct(r, J)
        else:
            rho0 = r @ r
        A = J.T @ J
        H[:lh.KC, :lh.KC] += A[:lh.KC, :lh.KC]
        g[:lh.KC] += J[:, :lh.KC].T @ r
        W += A[lh.KC, :lh.KC]
        a, b, cost = a + A[lh.KC, lh.KC], b + J[:, lh.KC] @ r, cost + 0.5 * rho0
    return H, g, a, b, W, cost


def _copy(lin):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lin.items()}


def _caught(stm, planted, cls, tag, table=None):
    """table: the comparators' own figures on this very window, where it belongs to no class of the case list"""
    rep = lh.report(stm, planted)
    bad = lh.failed_checks(rep, lh.ASSEMBLED_METRICS, cls) if table is None else [(k, rep[k], lh.MARGIN * table[k]) for k in lh.ASSEMBLED_METRICS
                                                                                   if not rep[k] <= lh.MARGIN * table[k]]
    print(f"{tag}: caught by " + (", ".join(f"{k} ({v:.3g} > {b:.3g})" for k, v, b in bad) or "NOTHING"))
    return bad


@pytest.mark.parametrize("name", ["n33", "prior_old"])
def test_planted_entry_errors_pass_the_flat_check_and_fail_the_new_ones(oracle, name):
    w, stm, cls = lc.window(oracle, name), statement(oracle, name), lc.case_class(name)
    good = oracle.linearize(w)
    assert lh.failed_checks(lh.report(stm, good), lh.ASSEMBLED_METRICS, cls) == []

    def largest(block):
        return np.unravel_index(np.argmax(np.abs(block)), block.shape)

    # 1e-9 in one entry of an (ex, pose_j) block
    p = _copy(good)
    i, j = largest(good["H"][66:72, 30:36])
    p["H"][66 + i, 30 + j] *= 1.0 + 1e-9
    p["H"][30 + j, 66 + i] = p["H"][66 + i, 30 + j]
    check_linearization(p, good)
    assert [b for b in _caught(stm, p, cls, f"{name}: 1e-9 in (ex, pose 5)") if b[0] == "H_ex"]
    # the same in the td entry of one landmark's W (the landmark whose td entry is the smallest that is still a tenth of its row)
    p = _copy(good)
    rows = np.abs(good["W"])
    ok = rows[:, 72] >= 0.1 * rows.max(axis=1)
    l = int(np.argmin(np.where(ok, rows[:, 72], np.inf)))
    assert ok[l] and rows[l, 72] < 0.1 * rows.max()
    p["W"][l, 72] *= 1.0 + 1e-9
    check_linearization(p, good)
    assert [b for b in _caught(stm, p, cls, f"{name}: 1e-9 in W[{l}, td]") if b[0] == "W_td"]
    # the same in one (pose_i, pose_j) block of frames that are not neighbours
    p = _copy(good)
    fi, fj = max(((a, b) for a in range(11) for b in range(a + 2, 11)), key=lambda ab: np.abs(good["H"][6 * ab[1]:6 * ab[1] + 6, 6 * ab[0]:6 * ab[0] + 6]).max())
    i, j = largest(good["H"][6 * fj:6 * fj + 6, 6 * fi:6 * fi + 6])
    p["H"][6 * fj + i, 6 * fi + j] *= 1.0 + 1e-9
    p["H"][6 * fi + j, 6 * fj + i] = p["H"][6 * fj + i, 6 * fi + j]
    check_linearization(p, good)
    assert [b for b in _caught(stm, p, cls, f"{name}: 1e-9 in (pose {fj}, pose {fi})") if b[0] == "H_pose_pose"]


def test_planted_factor_errors_pass_the_flat_check_and_fail_the_new_ones(oracle):
    w, big = close_point(oracle)
    stm, cls = lh.Statement(w), None
    good = oracle.linearize(w)
    print("close_point: largest entries", {k: f"{np.abs(good[k]).max():.1e}" for k in ("H", "g", "a", "b", "W")})
    # this window belongs to no class: its bars are 16 x the two comparators' own figures on it
    reps = [lh.report(stm, good), lh.report(stm, lh.comparator_np(w))]
    table = {m: max(r[m] for r in reps) for m in lh.ASSEMBLED_METRICS}
    print("close_point: comparators", {m: f"{v:.3g}" for m, v in table.items()})
    assert all(np.isfinite(v) for v in table.values())

    def caught(p, tag):
        return _caught(stm, p, cls, tag, table)
    k = np.diff(w.obs_offset)
    # one observation left out: the last one of a landmark with three or more
    l = int(next(x for x in range(w.N) if k[x] >= 3 and x != big))
    o = int(w.obs_offset[l + 1]) - 1
    off = w.obs_offset.copy()
    off[l + 1:] -= 1
    keep = np.arange(w.M) != o
    w1 = w.copy(obs_offset=off, obs_point=w.obs_point[keep], obs_velocity=w.obs_velocity[keep], obs_cur_td=w.obs_cur_td[keep], obs_uv_y=w.obs_uv_y[keep])
    p = oracle.linearize(w1)
    check_linearization(p, good)
    assert caught(p, f"observation {o} of landmark {l} left out")
    # one landmark's weight taken at s = 0
    l = int(next(x for x in range(w.N) if x != big))
    p = _copy(good)
    for sign, weighted in ((-1.0, True), (1.0, False)):
        H, g, a, b, W, cost = landmark_terms(w, l, weighted)
        p["H"] += sign * H
        p["g"] += sign * g
        p["a"][l] += sign * a
        p["b"][l] += sign * b
        p["W"][l] += sign * W
        p["cost"] += sign * cost
    check_linearization(p, good)
    assert caught(p, f"landmark {l} weighted at s = 0")
    # the td column replaced by the true derivative
    try:
        oracle.set_td_true_derivative(1)
        p = oracle.linearize(w)
    finally:
        oracle.set_td_true_derivative(0)
    check_linearization(p, good)
    assert [b for b in caught(p, "td column as the true derivative") if b[0] in ("H_td", "W_td", "g_td")]
