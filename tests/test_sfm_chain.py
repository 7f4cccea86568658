"""lfvio_sfm_construct (k_sfm_chain) against a 50-digit reference and against the numpy restatement (tests/sfm_chain_ref.py).

The fixtures tests/golden/sfm_chain_hp.npz hold one scene per case and, from the 50-digit side, every pose and position the chain
produces; tests/golden/gen_sfm_chain_hp.py writes them, lists the cases and asserts the conditions under which the chain's discrete
decisions (the sign pins of the control points, which singular vector is the smallest) are safe.  Metrics, in units of eps = 2^-52:

  R     largest |difference| of an entry of the rotation matrices of c_rotation (of q / |q|: q and -q are one rotation), over the frames
  t, X  largest |difference| of an entry of c_translation / position, relative to the largest |entry| of the fixture's
  ba    (hand-over, noisy cases) |final_cost - the fixture's| / the fixture's, where the fixture's is sfm_ba_ref.solve (double precision,
        default options) started from the 50-digit chain's result

tri_op, pnp_op, pnp_count, num_triangulated and status are held exactly.

BARS.  bar = 16 x the worst value the numpy restatement reaches against the same 50-digit fixtures, per metric and regime, floor 2, as
tests/test_pnp.py and tests/test_sfm_ba.py have it; REF below is that measurement (rounded up to two digits) and
tests/test_sfm_chain_ref.py re-measures it.  For `ba` the restatement's value is its own chain into sfm_ba_ref.solve, the worst over three
listings of the scene's points (as stored, reversed, shuffled: the same mathematics, other rounding — on the stored listing alone the
restatement and the fixture's value share sfm_ba_ref's summation order and its rounding cancels).  The regimes: f2
(F = 2, no PnP), f3 (F = 3, l = 0 and 1), f11_noisy / f11_exact (F = 11, P = 60, l = 0, 5, 9), ragged (F = 6, l = 2), big (F = 4, P = 257
and 4096).  The errors of a chain grow with every PnP (each is EPnP's own: pnp_ref's 57 ... 4e6 eps) and triangulation on top of it;
the noisy regimes are the large ones.

worst restatement / bar / worst device (MI355X), per regime
  regime     R                  t                  X                  ba
  f2         0.13/2.08/0.13     0.51/8.16/0.5      39/624/2.4         120/1920/15
  f3         14/224/2.2         63/1008/9.3        180/2880/7.7       25/400/18
  f11_noisy  38/608/11          41/656/22          270/4320/107       5.3/84.8/6
  f11_exact  34/544/7.3         40/640/12          130/2080/69        -
  ragged     11/176/2.9         40/640/12          94/1504/30         6.3/101/5.6
  big        4.9/78.4/1.9       30/480/17          230/3680/52        1.9/30.4/1.8
(ragged includes the stopped chain of test (e).)
"""
import ctypes as C
import os

import numpy as np
import pytest

import pnp_ref as pr
import sfm_ba_ref as sr
import sfm_chain_ref as cr
from golden import gen_sfm_chain_hp as gen

EPS = 2.0 ** -52
FACTOR, FLOOR = 16.0, 2.0
CASES = tuple(gen.CASES)
REGIME = gen.REGIME
REGIMES = ("f2", "f3", "f11_noisy", "f11_exact", "ragged", "big")
NOISY = gen.NOISY
STOPPED = tuple(gen.STOPPED)
QUAT_BAR = 4.0  # (b): c_rotation against the stated conversion of out.pnp[f].R, in eps (reasoned in that test)

# worst value of the numpy restatement against the 50-digit fixtures, per regime (rounded up to two digits)
REF = {
    "f2": dict(R=0.13, t=0.51, X=39, ba=1.2e+02),
    "f3": dict(R=14, t=63, X=1.8e+02, ba=25),
    "f11_noisy": dict(R=38, t=41, X=2.7e+02, ba=5.3),
    "f11_exact": dict(R=34, t=40, X=1.3e+02),
    "ragged": dict(R=11, t=40, X=94, ba=6.3),
    "big": dict(R=4.9, t=30, X=2.3e+02, ba=1.9),
}


def bar(case, metric):
    return max(FACTOR * REF[REGIME[case]][metric], FLOOR)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "sfm_chain_hp.npz"))
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["names"]}


def args_of(f):
    return (int(f["F"]), int(f["l"]), f["off"], f["frame"], f["bearing"], f["relative_R"], f["relative_T"])


def restatement(f):
    r = cr.construct(*args_of(f))
    return dict(r, c_rotation=np.asarray(r["c_rotation"], np.float64), c_translation=np.asarray(r["c_translation"], np.float64),
                position=np.asarray(r["position"], np.float64))


def metrics(got, f):
    tri, posed = f["tri_op"] >= 0, f["posed"]  # (a chain that stops leaves frames unposed and points untriangulated)
    return dict(R=float(np.abs(cr.rotation_of(got["c_rotation"][posed]) - cr.rotation_of(f["c_rotation"][posed])).max() / EPS),
                t=float(np.abs(got["c_translation"][posed] - f["c_translation"][posed]).max() / (EPS * np.abs(f["c_translation"][posed]).max())),
                X=float(np.abs(got["position"][tri] - f["position"][tri]).max() / (EPS * np.abs(f["position"][tri]).max())))


def discrete_equal(got, f):
    return (got["status"] == int(f["status"]) and got["failed_frame"] == int(f["failed_frame"]) and got["num_triangulated"] == int(f["num_triangulated"]) and np.array_equal(got["tri_op"], f["tri_op"])
            and np.array_equal(got["pnp_op"], f["pnp_op"]) and np.array_equal(got["pnp_count"], f["pnp_count"]))


def hand_over(got, f, ba):
    """The chain's result compacted into a bundle adjustment (`ba`: the device's or the restatement's) -> its result."""
    cp = cr.compact(got, f["off"], f["frame"], f["bearing"])
    return ba(int(f["F"]), int(f["l"]), cp, got["c_rotation"], got["c_translation"])


def ba_restatement(F, l, cp, q, t):
    return sr.solve(sr.problem(F, l, cp["off"], cp["frame"], cp["bearing"]), q, t, cp["position"])


def ba_metric(res, f):
    return float(abs(res["final_cost"] - float(f["ba_final_cost"])) / (EPS * float(f["ba_final_cost"])))


def listings(f):
    """Three orders of the points of one scene: as stored, reversed, shuffled.  The same mathematics, other rounding."""
    P = len(f["off"]) - 1
    return [np.arange(P), np.arange(P)[::-1], np.random.default_rng(1).permutation(P)]


def relisted(f, perm):
    """The scene with its points listed in the order perm."""
    off = f["off"]
    order = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm])
    return dict(f, off=np.concatenate([[0], np.cumsum(np.diff(off)[perm])]).astype(np.int32), frame=f["frame"][order], bearing=f["bearing"][order])


def measure_restatement(fx):
    """Per regime, the worst over its cases of the restatement's error against the 50-digit fixture; for `ba`, the worst over three listings
    of the scene's points (as tests/test_sfm_ba.py measures its trace: on one listing the restatement and the fixture's value share
    sfm_ba_ref's summation order, and its rounding would cancel)."""
    out = {}
    for case in CASES + STOPPED:
        f = fx[case]
        got = restatement(f)
        assert discrete_equal(got, f), case
        m = metrics(got, f)
        if case in NOISY:
            m["ba"] = max(ba_metric(hand_over(restatement(g), g, ba_restatement), f) for g in (relisted(f, p) for p in listings(f)))
        r = out.setdefault(REGIME[case], {})
        for k, v in m.items():
            r[k] = max(r.get(k, 0.0), v)
    return out


def check(m, case, tag):
    bad = [f"{tag} {case} {k}: {v:.3g} > bar {bar(case, k):.3g}" for k, v in m.items() if not v <= bar(case, k)]
    assert not bad, "\n".join(bad)


def show(tag, case, m):
    print(f"  {tag} {case:14s} " + " ".join(f"{k} {v:9.3g}" for k, v in m.items()))


def device(eng, f, **kw):
    return eng.sfm_construct(*args_of(f), **kw)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_a_accuracy(eng, fixtures, case):
    """(a): poses and positions against the 50-digit fixture; tri_op, pnp_op, pnp_count, num_triangulated and status exactly; a point that
    stays untriangulated has position 0, 0, 0."""
    f = fixtures[case]
    got = device(eng, f)
    assert discrete_equal(got, f), case
    assert got["failed_frame"] == -1 and not np.any(got["position"][got["tri_op"] < 0])
    m = metrics(got, f)
    show("device (a)", case, m)
    check(m, case, "(a)")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_b_pnp_drop_in_identity(eng, fixtures, case):
    """(b): for every frame with pnp_op >= 0, lfvio_pnp on the points with 0 <= tri_op[j] < pnp_op[f] observed in f, in ascending j, with the
    call's final positions (a position never changes once set) returns out.pnp[f]'s R, T and err bit for bit.  c_translation is that T bit
    for bit; c_rotation is Eigen's matrix to quaternion conversion of that R, restated in numpy.  An entry of the unit quaternion is at most
    five rounded operations from the entries of R (the sum, + 1, the square root, 0.5 / t, the product) and at most 1 in size: the two
    sides are within 5 half-units = 2.5 eps where their operations round alike or not; QUAT_BAR = 4 eps."""
    f = fixtures[case]
    F, off = int(f["F"]), f["off"]
    got = device(eng, f)
    for fr in range(F):
        if got["pnp_op"][fr] < 0:
            assert fr in (int(f["l"]), F - 1) and not np.any(got["pnp"][fr]["R"]), (case, fr)
            continue
        js = [j for j in range(len(off) - 1) if 0 <= got["tri_op"][j] < got["pnp_op"][fr] and fr in f["frame"][off[j]:off[j + 1]]]
        us = np.array([f["bearing"][off[j] + list(f["frame"][off[j]:off[j + 1]]).index(fr)] for j in js])
        assert len(js) == got["pnp_count"][fr], (case, fr)
        one = eng.pnp([0, len(js)], got["position"][js], us)[0]
        rec = got["pnp"][fr]
        assert one["status"] == 0 and rec["status"] == 0
        for k in ("R", "T", "err"):
            assert one[k].tobytes() == rec[k].tobytes(), (case, fr, k)
        assert got["c_translation"][fr].tobytes() == rec["T"].tobytes(), (case, fr)
        q = np.asarray(cr.quat_of_matrix(rec["R"], pr.F64), np.float64)
        assert np.abs(got["c_rotation"][fr] - q).max() <= QUAT_BAR * EPS, (case, fr, np.abs(got["c_rotation"][fr] - q).max() / EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOISY)
def test_c_hand_over_to_the_bundle_adjustment(eng, fixtures, case):
    """(c): the outputs, compacted, go into Engine.sfm_ba under default options: accepted = 1, and the final cost within 16 x the error of
    the restatement's chain into sfm_ba_ref.solve."""
    f = fixtures[case]
    got = device(eng, f)
    res = hand_over(got, f, lambda F, l, cp, q, t: eng.sfm_ba(l, cp["off"], cp["frame"], cp["bearing"], q, t, cp["position"]))
    assert len(res["position"]) == got["num_triangulated"]
    m = dict(ba=ba_metric(res, f))
    show("device (c)", case, m)
    assert res["accepted"] == 1 and int(f["ba_accepted"]) == 1, case
    check(m, case, "(c)")


@pytest.mark.gpu
def test_d_repeated_call_returns_the_same_bits(eng, fixtures):
    for case in ("f3_p12_l1", "f11_l5", "ragged", "f4_p4096"):
        a, b = device(eng, fixtures[case]), device(eng, fixtures[case])
        for k in ("c_rotation", "c_translation", "position", "tri_op", "pnp_op", "pnp_count"):
            assert a[k].tobytes() == b[k].tobytes(), (case, k)
        assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a["pnp"], b["pnp"]) for k in ("R", "T", "err")), case


@pytest.mark.gpu
def test_e_status_1_stops_the_chain(eng, fixtures):
    """(e): the ragged scene without one full track: the PnP of frame 0 gets 9 correspondences.  Status 1 and failed_frame 0; the frames
    before it in the schedule (2, 5, 3, 4, 1) are posed, to the bars of (a) against the 50-digit run of the same stopped chain; the rows of
    frame 0 keep what the caller had and its record stays zero; the points triangulated by then keep their op (the last is op 8), the
    others are -1 and 0, 0, 0."""
    f = fixtures["ragged_short"]
    assert int(f["status"]) == 1 and int(f["failed_frame"]) == 0 and list(f["posed"]) == [False, True, True, True, True, True]
    q, t = np.full((6, 4), 7.5), np.full((6, 3), -7.5)
    got = device(eng, f, c_rotation=q, c_translation=t)
    assert discrete_equal(got, f) and got["pnp_count"][0] == 9 and got["pnp_op"][0] == 9 and got["tri_op"].max() == 8
    assert np.all(q[0] == 7.5) and np.all(t[0] == -7.5) and not np.any(got["pnp"][0]["R"]) and not np.any(q[1:] == 7.5)
    assert not np.any(got["position"][got["tri_op"] < 0]) and np.any(got["tri_op"] < 0)
    m = metrics(got, f)
    show("device (e)", "ragged_short", m)
    check(m, "ragged_short", "(e)")


def filled():
    from lfvio import abi

    out = abi.SfmConstructOutC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return out


@pytest.mark.gpu
def test_f_errors_leave_the_outputs_alone(eng, fixtures):
    """(f): every LFVIO_ERR_ARG row of the header."""
    from lfvio import abi

    f = fixtures["f3_p12_l0"]
    F, l, off, frm, us, R, T = args_of(f)
    big = 4097
    twice = frm.copy()
    twice[1] = twice[0]
    bad_off = off.copy()
    bad_off[2] = bad_off[1]
    cases = {
        "F = 1": (1, 0, [0, 1], [0], us[:1]),
        "F = 12": (12, 0, off, frm, us),
        "l = -1": (F, -1, off, frm, us),
        "l = F - 1": (F, 2, off, frm, us),
        "P = 4097": (F, l, np.arange(big + 1), np.zeros(big, np.int32), np.tile(us[:1], (big, 1))),
        "offset[0] != 0": (F, l, off + 1, frm, np.concatenate([us[:1], us])),
        "a point with no observation": (F, l, bad_off, frm, us),
        "a point with F + 1": (F, l, [0, 4], [0, 1, 2, 1], us[:4]),
        "frame = F": (F, l, off, np.where(np.arange(len(frm)) == 5, 3, frm), us),
        "frame = -1": (F, l, off, np.where(np.arange(len(frm)) == 5, -1, frm), us),
        "a frame twice": (F, l, off, twice, us),
    }
    for tag, (F_, l_, o_, f_, u_) in cases.items():
        out = filled()
        before = bytes(out)
        P_ = len(o_) - 1
        q, t, X, ops = np.full((12, 4), 1.5), np.full((12, 3), 2.5), np.full((P_, 3), 3.5), np.full(P_, 77, np.int32)
        got = eng.sfm_construct(F_, l_, o_, f_, u_, R, T, c_rotation=q, c_translation=t, position=X, tri_op=ops, out=out, check=False)
        assert got["rc"] == -1 and bytes(out) == before, tag
        assert np.all(q == 1.5) and np.all(t == 2.5) and np.all(X == 3.5) and np.all(ops == 77), tag
    # null pointers
    out = filled()
    before = bytes(out)
    P = len(off) - 1
    q, t, X, ops = np.full((F, 4), 1.5), np.full((F, 3), 2.5), np.full((P, 3), 3.5), np.full(P, 77, np.int32)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    cin = abi.SfmConstructInC()
    cin.num_frames, cin.ref_frame, cin.num_points = F, l, P
    call = eng.lib.lfvio_sfm_construct
    assert call(eng.ctx, C.byref(cin), dp(q), dp(t), dp(X), ip(ops), C.byref(out)) == -1  # null arrays
    o32, f32 = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(frm, np.int32)
    cin.obs_offset, cin.obs_frame, cin.obs_bearing = ip(o32), ip(f32), dp(us)
    assert call(eng.ctx, None, dp(q), dp(t), dp(X), ip(ops), C.byref(out)) == -1
    assert call(eng.ctx, C.byref(cin), None, dp(t), dp(X), ip(ops), C.byref(out)) == -1
    assert call(eng.ctx, C.byref(cin), dp(q), None, dp(X), ip(ops), C.byref(out)) == -1
    assert call(eng.ctx, C.byref(cin), dp(q), dp(t), None, ip(ops), C.byref(out)) == -1
    assert call(eng.ctx, C.byref(cin), dp(q), dp(t), dp(X), None, C.byref(out)) == -1
    assert call(eng.ctx, C.byref(cin), dp(q), dp(t), dp(X), ip(ops), None) == -1
    assert bytes(out) == before and np.all(q == 1.5) and np.all(t == 2.5) and np.all(X == 3.5) and np.all(ops == 77)
    assert device(eng, f)["status"] == 0  # the context is still good
