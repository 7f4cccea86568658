"""k_triangulate, k_shift_depth and k_preintegrate against a 50-digit reference: per landmark, per 3x3 block.

The fixtures tests/golden/{preint,triangulate,shift}_hp.npz hold inputs and the results of tests/hp_ref.py (mpmath,
50 digits) rounded to double; tests/golden/gen_feature_hp.py writes them.  Every metric is relative to what it measures:

  pre-integration   each of the 25 3x3 blocks of jacobian and covariance: max|got - ref| / max|ref| over the block;
                    delta_p, delta_v per vector; delta_q absolute and | |q| - 1 |; sum_dt bit-equal to the oracle's;
                    the structural zeros and identities exact
  triangulation     per landmark |got - ref| / |ref| in units of eps sigma_1/sigma_4 of that landmark's system
  shift depth       per landmark |got - ref| in units of eps (|depth| |uv| + |marg_P| + |new_P|)

BARS.  bar = 16 x the worst value the double-precision restatements (the C++ oracle, and numpy: synth.preintegrate,
np_ref.triangulate, np_ref.shift_depth) reach against the same fixtures, per metric and per regime, floor 2 eps (2 in
eps units).  REF below is that measurement (test_restatements_* re-measure it and hold them to it); the device columns
are the worst values of the MI355X run this table was filled from.  Jacobian and covariance: worst block of the regime.

pre-integration: worst restatement / bar / worst device, per regime (cases of tests/golden/gen_feature_hp.py)
  regime    delta_p                    delta_v                    delta_q (abs)              | |q| - 1 |                jacobian, worst block      covariance, worst block
  usual     4.9e-16/7.8e-15/4.8e-16    5.6e-16/9.0e-15/5.5e-16    1.2e-16/1.9e-15/2.2e-16    2.3e-16/3.7e-15/2.2e-16    1.6e-15/2.6e-14/1.5e-15    4.8e-15/7.7e-14/3.3e-15
  fast      7.9e-16/1.3e-14/1.2e-15    7.9e-16/1.3e-14/3.9e-16    1.4e-15/2.2e-14/7.8e-16    1.2e-16/1.9e-15/1.1e-16    2.3e-15/3.7e-14/2.1e-15    2.6e-15/4.2e-14/2.0e-15
  bias      2.1e-16/3.4e-15/2.1e-16    3.6e-16/5.8e-15/3.5e-16    2.5e-16/4.0e-15/1.1e-16    0.0e+00/4.4e-16/1.1e-16    1.4e-15/2.2e-14/1.3e-15    2.8e-15/4.5e-14/3.2e-15
  dt0_mid   7.4e-16/1.2e-14/7.4e-16    9.2e-16/1.5e-14/9.2e-16    1.2e-16/1.9e-15/1.0e-17    0.0e+00/4.4e-16/1.1e-16    1.2e-15/1.9e-14/1.1e-15    2.8e-15/4.5e-14/2.5e-15
  dt0_first 1.5e-15/2.4e-14/1.5e-15    4.3e-16/6.9e-15/4.3e-16    1.2e-16/1.9e-15/1.1e-16    1.2e-16/1.9e-15/1.1e-16    2.8e-15/4.5e-14/2.8e-15    3.0e-15/4.8e-14/1.7e-15
  noise0    3.8e-16/6.1e-15/3.7e-16    2.9e-16/4.6e-15/2.9e-16    1.5e-16/2.4e-15/2.2e-16    1.2e-16/1.9e-15/2.2e-16    1.9e-15/3.0e-14/1.9e-15    0 / exact / 0
  noise2    3.7e-16/5.9e-15/3.7e-16    2.9e-16/4.6e-15/2.9e-16    1.2e-16/1.9e-15/1.1e-16    1.2e-16/1.9e-15/1.1e-16    2.3e-15/3.7e-14/2.2e-15    4.1e-15/6.6e-14/2.8e-15
  (no block of any regime exceeds 100 eps on the reference side, so none has a row of its own; the exact structure —
  zeros, identities, sum_dt, biases — held bit for bit on the device in every case.  600 ragged intervals against the
  oracle, bars + the oracle's worst: delta_p 1.4e-16, delta_v 1.4e-16, delta_q 3.4e-16, jacobian 8.6e-16, covariance 3.1e-15.)
triangulation [eps sigma_1/sigma_4 of the landmark]: worst restatement / bar / worst device
  window 22/352/7.74   pairs 9.1/145.6/0.78   lowpar_0.01 11/176/4.12   lowpar_0.001 1.2/19.2/0.34   lowpar_0.0001 1.4/22.4/0.04   mirror 5.3/84.8/0.95
  (window = make_window(0, 300) and (3, 60); sizes 1 .. 5000 against the oracle, bar 352 + 22: worst 38.8 at N = 5000)
shift depth [eps (|depth| |uv| + |marg_P| + |new_P|)]: worst restatement / bar / worst device
  ordinary_n1 0/2/0   ordinary_n255 1.6/25.6/1.79   ordinary_n256 2/32/1.52   ordinary_n257 1.7/27.2/1.52   ordinary_n5000 1.8/28.8/1.75
  far_n257 0.19/3.04/0.19   cancel_n257 0.25/4/0.31   zero_n300 1.3/20.8/1.54
"""
import os

import numpy as np
import pytest

import np_ref
from golden import gen_feature_hp as gen
from lfvio import abi, synth

EPS = 2.0 ** -52
FACTOR = 16.0
NOISE = gen.NOISE
BLK = ["p", "th", "v", "ba", "bg"]

# worst value of each metric over the oracle and the numpy restatement, per regime (rounded up to two digits)
REF_PRE = {
    "usual": dict(dp=4.9e-16, dv=5.6e-16, dq=1.2e-16, qn=2.3e-16, J=1.6e-15, P=4.8e-15),
    "fast": dict(dp=7.9e-16, dv=7.9e-16, dq=1.4e-15, qn=1.2e-16, J=2.3e-15, P=2.6e-15),
    "bias": dict(dp=2.1e-16, dv=3.6e-16, dq=2.5e-16, qn=0.0, J=1.4e-15, P=2.8e-15),
    "dt0_mid": dict(dp=7.4e-16, dv=9.2e-16, dq=1.2e-16, qn=0.0, J=1.2e-15, P=2.8e-15),
    "dt0_first": dict(dp=1.5e-15, dv=4.3e-16, dq=1.2e-16, qn=1.2e-16, J=2.8e-15, P=3.0e-15),
    "noise0": dict(dp=3.8e-16, dv=2.9e-16, dq=1.5e-16, qn=1.2e-16, J=1.9e-15, P=0.0),
    "noise2": dict(dp=3.7e-16, dv=2.9e-16, dq=1.2e-16, qn=1.2e-16, J=2.3e-15, P=4.1e-15),
}
# blocks whose reference-side error exceeds ~100 eps in some regime get a row of their own: {(regime, "J"|"P", row, col): worst}
REF_PRE_BLOCK = {}  # none: the worst block of any regime is at 22 eps
REF_TRI = {  # eps sigma_1/sigma_4 units
    "window": 22.0, "pairs": 9.1, "lowpar_0.01": 11.0, "lowpar_0.001": 1.2, "lowpar_0.0001": 1.4, "mirror": 5.3,
}
REF_SHIFT = {  # eps (|depth| |uv| + |marg_P| + |new_P|) units
    "ordinary_n1": 0.0, "ordinary_n255": 1.6, "ordinary_n256": 2.0, "ordinary_n257": 1.7, "ordinary_n5000": 1.8,
    "far_n257": 0.19, "cancel_n257": 0.25, "zero_n300": 1.3,
}
# factor 16 everywhere; a metric whose device rounding is legitimately larger may be listed here with at most 64 and its reason
FACTOR_OF = {}


def bar(worst, floor=2 * EPS, factor=FACTOR):
    return max(factor * worst, floor)


def pre_bar(regime, what, blk=None):
    if blk is not None and (regime, what) + blk in REF_PRE_BLOCK:
        return bar(REF_PRE_BLOCK[(regime, what) + blk], factor=FACTOR_OF.get((regime, what) + blk, FACTOR))
    return bar(REF_PRE[regime][what], factor=FACTOR_OF.get((regime, what), FACTOR))


def tri_regime(group):
    return "window" if group.startswith("w") else group


def blk(a, i, j):
    return a[3 * i:3 * i + 3, 3 * j:3 * j + 3]


def pre_metrics(got, ref):
    """{metric: value} of one interval; got, ref the 467 doubles of abi.preint_to_array.  Blocks that are zero in the
    reference are exact zeros by structure: any non-zero there gives inf."""
    m = {"dp": np.abs(got[1:4] - ref[1:4]).max() / np.abs(ref[1:4]).max(),
         "dv": np.abs(got[8:11] - ref[8:11]).max() / np.abs(ref[8:11]).max(),
         "dq": np.abs(got[4:8] - ref[4:8]).max(), "qn": abs(np.linalg.norm(got[4:8]) - 1.0)}
    for what, o in (("J", 17), ("P", 242)):
        G, R = got[o:o + 225].reshape(15, 15), ref[o:o + 225].reshape(15, 15)
        for i in range(5):
            for j in range(5):
                g, r = blk(G, i, j), blk(R, i, j)
                m[(what, BLK[i], BLK[j])] = np.abs(g - r).max() / np.abs(r).max() if r.any() else (np.inf if g.any() else 0.0)
    return m


def pre_check(tag, regime, got, ref, extra=None):
    """Every metric of one interval against its bar (+ extra[what]: the reference's own error where `ref` is the oracle).
    Returns the metrics; the message names interval, block, value and bar."""
    m = pre_metrics(got, ref)
    bad = []
    for k, v in m.items():
        what = k if isinstance(k, str) else k[0]
        b = pre_bar(regime, what, None if isinstance(k, str) else k[1:]) + (extra[what] if extra else 0.0)
        if not v <= b:
            bad.append(f"{tag} {k}: {v:.3e} > bar {b:.3e}")
    assert not bad, "\n".join(bad)
    return m


def pre_structure(tag, a, noise):
    """The exact part: identities and zeros that no rounding can touch."""
    J, P = a[17:242].reshape(15, 15), a[242:].reshape(15, 15)
    Z, I = np.zeros((3, 3)), np.eye(3)
    for i in range(5):
        assert np.array_equal(blk(J, i, 0), I if i == 0 else Z), f"{tag} J[{BLK[i]},p]"
    for i in (3, 4):  # rows ba, bg: identity rows
        for j in range(5):
            assert np.array_equal(blk(J, i, j), I if i == j else Z), f"{tag} J[{BLK[i]},{BLK[j]}]"
    for j in (0, 2, 3):  # the theta row is zero outside (th, th) and (th, bg)
        assert np.array_equal(blk(J, 1, j), Z), f"{tag} J[th,{BLK[j]}]"
    for i, j in ((1, 3), (3, 1), (3, 4), (4, 3)):
        assert np.array_equal(blk(P, i, j), Z), f"{tag} P[{BLK[i]},{BLK[j]}]"
    if not np.any(noise):
        assert not P.any(), f"{tag} covariance with zero noise"


def pre_cov_checks(tag, regime, a, ref):
    """Symmetry within the bar of the block, and the scaled covariance positive semi-definite within 15 bars."""
    P, R = a[242:].reshape(15, 15), ref[242:].reshape(15, 15)
    for i in range(5):
        for j in range(i, 5):
            d = np.abs(blk(P, i, j) - blk(P, j, i).T).max()
            assert d <= pre_bar(regime, "P", (BLK[i], BLK[j])) * np.abs(blk(R, i, j)).max(), f"{tag} P[{BLK[i]},{BLK[j]}] asymmetric by {d:.3e}"
    keep = np.diag(P) > 0
    assert np.array_equal(keep, np.diag(R) > 0), f"{tag} zero rows of the covariance"
    if keep.any():
        s = 1.0 / np.sqrt(np.diag(P)[keep])
        C = P[np.ix_(keep, keep)] * s[:, None] * s[None, :]
        lo = np.linalg.eigvalsh(0.5 * (C + C.T)).min()
        assert lo >= -15 * pre_bar(regime, "P"), f"{tag} smallest eigenvalue of the scaled covariance {lo:.3e}"


def fold(worst, m):
    for k, v in m.items():
        what = k if isinstance(k, str) else k[0]
        if v >= worst.get(what, (-1.0, None))[0]:
            worst[what] = (v, k)


def tri_systems(g):
    """sigma_1 / sigma_4 per landmark (numpy; for inputs that have no fixture)."""
    c = np.zeros(len(g.start_frame))
    for l in range(len(c)):
        i, o0, o1 = int(g.start_frame[l]), int(g.obs_offset[l]), int(g.obs_offset[l + 1])
        t0, R0 = g.Ps[i] + g.Rs[i] @ g.tic, g.Rs[i] @ g.ric
        rows = []
        for o in range(o1 - o0):
            t1, R1 = g.Ps[i + o] + g.Rs[i + o] @ g.tic, g.Rs[i + o] @ g.ric
            R = R0.T @ R1
            P = np.hstack([R.T, (-R.T @ (R0.T @ (t1 - t0)))[:, None]])
            f = g.obs_point[o0 + o] / np.linalg.norm(g.obs_point[o0 + o])
            rows += [f[0] * P[2] - f[2] * P[0], f[1] * P[2] - f[2] * P[1]]
        s = np.linalg.svd(np.array(rows), compute_uv=False)
        c[l] = s[0] / s[3]
    return c


def tri_metric(got, ref, cond):
    return np.abs(got - ref) / np.abs(ref) / (EPS * cond)


def tri_check(tag, got, g, ref_bar):
    """One stored group: decisions equal, untouched depths bit for bit, the rest per landmark.  Returns the worst metric."""
    want, init = g["depth_out"], float(g["init_depth"])
    keep = g["depth_in"] > 0
    assert np.array_equal(got[keep], g["depth_in"][keep]), f"{tag}: a positive depth was touched"
    behind = (g["d_raw"] < 0) & ~keep
    assert np.array_equal((got == init) & ~keep, behind), f"{tag}: init_depth decision differs at {np.flatnonzero(((got == init) & ~keep) != behind)}"
    assert np.array_equal(got[behind], want[behind])
    m = tri_metric(got, want, g["sigma"][:, 0] / g["sigma"][:, 3])
    m[keep | behind] = 0.0
    bad = np.flatnonzero(~(m <= ref_bar))
    assert len(bad) == 0, "\n".join(f"{tag} landmark {l} (start {g['start_frame'][l]}, k {g['obs_offset'][l + 1] - g['obs_offset'][l]}, "
                                    f"sigma1/sigma4 {g['sigma'][l, 0] / g['sigma'][l, 3]:.1e}): {m[l]:.2f} > bar {ref_bar:.2f} [eps cond]"
                                    for l in bad[:10])
    return m.max()


def shift_metric(got, c):
    terms = np.abs(c["depth"]) * np.linalg.norm(c["uv"], axis=1) + np.linalg.norm(c["marg_P"]) + np.linalg.norm(c["new_P"])
    return np.abs(got - c["out"]) / (EPS * terms)


def shift_check(tag, got, c, ref_bar):
    zero = (c["depth"] == 0) & np.array_equal(c["marg_P"], c["new_P"])
    assert np.array_equal(got[zero], np.full(int(zero.sum()), float(c["init_depth"]))), f"{tag}: init_depth entries"
    m = shift_metric(got, c)
    bad = np.flatnonzero(~(m <= ref_bar))
    assert len(bad) == 0, "\n".join(f"{tag} landmark {l}: {m[l]:.2f} > bar {ref_bar:.2f} [eps terms]" for l in bad[:10])
    return m.max()


@pytest.fixture(scope="module")
def pre_cases(golden_dir):
    return gen.load_preint(os.path.join(golden_dir, "preint_hp.npz"))


@pytest.fixture(scope="module")
def tri_groups(golden_dir):
    return gen.load_triangulate(os.path.join(golden_dir, "triangulate_hp.npz"))


@pytest.fixture(scope="module")
def shift_cases(golden_dir):
    return gen.load_shift(os.path.join(golden_dir, "shift_hp.npz"))


PRE_IDS = [f"{c[0]}-n{c[1]}" for c in gen.pre_case_list()]
TRI_IDS = ["w0_300", "w3_60", "pairs"] + [f"lowpar_{p:g}" for p in gen.TRI_LOW_PARALLAX] + ["mirror"]
SHIFT_IDS = [f"ordinary_n{n}" for n in (1, 255, 256, 257, 5000)] + ["far_n257", "cancel_n257", "zero_n300"]


# ----------------------------------------------------------------------------------------------------------------
# CPU: the files belong to the generator, and the restatements define the bars
# ----------------------------------------------------------------------------------------------------------------
def test_fixture_lists_are_the_generators(pre_cases, tri_groups, shift_cases):
    assert [c[0] for c in pre_cases] == PRE_IDS and list(tri_groups) == TRI_IDS and list(shift_cases) == SHIFT_IDS
    assert {c[2] % 8 for c in pre_cases} == set(range(8))
    for case, (tag, _, _, noise, iv, _) in zip(gen.pre_case_list(), pre_cases):  # the stored inputs are the seeded ones
        assert np.array_equal(noise, case[3])
        for a, b in zip(iv, gen.pre_interval(case)):
            assert np.array_equal(a, b), tag
    live = gen.tri_groups()
    for name, g in tri_groups.items():
        for k, v in live[name].items():
            assert np.array_equal(g[k], v), (name, k)
        cond = g["sigma"][:, 0] / g["sigma"][:, 3]
        assert cond.max() <= gen.TRI_MAX_COND
        # no bar of this file reaches the sign of any stored d: the init_depth decision is unambiguous
        assert (np.abs(g["d_raw"]) > 1e3 * gen.TRI_SIGN_BAR * EPS * cond * g["scale"]).all()
    assert max(bar(v, floor=2.0) for v in REF_TRI.values()) + max(REF_TRI.values()) <= gen.TRI_SIGN_BAR
    k = np.diff(tri_groups["pairs"]["obs_offset"])
    pairs = list(zip(tri_groups["pairs"]["start_frame"], k))
    assert all(pairs.count((s, n)) >= 2 for s in range(10) for n in range(2, 12 - s))
    for g in ("w0_300", "w3_60"):
        assert (tri_groups[g]["depth_in"][::3] > 0).all()
    live = gen.shift_cases()
    for name, c in shift_cases.items():
        for k, v in live[name].items():
            assert np.array_equal(c[k], v), (name, k)


def test_fixtures_rerun_live(pre_cases, tri_groups, shift_cases):
    """A few small stored cases through the 50-digit code again: 53 samples, 12 landmarks, 20 shifted depths."""
    pytest.importorskip("mpmath")
    cases = gen.pre_case_list()
    small = [k for k, c in enumerate(cases) if c[0] == "usual" and c[1] <= 15]
    assert sum(cases[k][1] for k in small) <= 60
    for k in small:
        assert np.array_equal(gen.pre_expected(cases[k]), pre_cases[k][5]), pre_cases[k][0]
    for name, idx in (("w3_60", [1, 2, 4, 5]), ("pairs", [0, 9, 54, 109]), ("lowpar_0.0001", [0, 7]), ("mirror", [0, 1])):
        g = tri_groups[name]
        out, raw, sig, sc = gen.tri_expected(g, only=idx)
        assert np.array_equal(out, g["depth_out"][idx]) and np.array_equal(raw, g["d_raw"][idx]), name
        assert np.array_equal(sig, g["sigma"][idx]) and np.array_equal(sc, g["scale"][idx]), name
    for name, sl in (("ordinary_n1", slice(0, 1)), ("cancel_n257", slice(0, 5)), ("far_n257", slice(250, 257)), ("zero_n300", slice(252, 259))):
        assert np.array_equal(gen.shift_expected(shift_cases[name], sl), shift_cases[name]["out"][sl]), name


def measure_restatements_preint(pre_cases, oracle):
    """{regime: {metric: (worst, where)}} over the oracle and synth.preintegrate, and the blocks beyond 100 eps."""
    worst, big = {}, {}
    for tag, regime, n, noise, (ba, bg, a0, g0, dts, accs, gyrs), ref in pre_cases:
        for name, fn in (("oracle", oracle.preintegrate), ("numpy", synth.preintegrate)):
            a = abi.preint_to_array(fn(a0, g0, ba, bg, dts, accs, gyrs, noise))
            pre_structure(f"{name} {tag}", a, noise)
            assert np.array_equal(a[11:17], ref[11:17])
            m = pre_metrics(a, ref)
            fold(worst.setdefault(regime, {}), {k: v for k, v in m.items() if isinstance(k, str) or (regime,) + k not in REF_PRE_BLOCK})
            for k, v in m.items():
                if not isinstance(k, str) and v > 100 * EPS:
                    big[(regime,) + k] = max(big.get((regime,) + k, 0.0), v)
    return worst, big


def test_restatements_preintegration(pre_cases, oracle):
    worst, big = measure_restatements_preint(pre_cases, oracle)
    for regime, w in worst.items():
        print(regime, {k: f"{v[0]:.2e} {v[1]}" for k, v in w.items()})
        for what, (v, where) in w.items():
            assert v <= REF_PRE[regime][what], (regime, what, where, v)
    print("blocks beyond 100 eps:", big)
    for k, v in big.items():
        assert k in REF_PRE_BLOCK and v <= REF_PRE_BLOCK[k], (k, v)
    # sum_dt: the oracle and numpy add the same doubles in the same order
    for tag, _, _, noise, (ba, bg, a0, g0, dts, accs, gyrs), ref in pre_cases:
        s = oracle.preintegrate(a0, g0, ba, bg, dts, accs, gyrs, noise).sum_dt
        assert s == synth.preintegrate(a0, g0, ba, bg, dts, accs, gyrs, noise).sum_dt and abs(s - ref[0]) <= len(dts) * EPS * ref[0]  # n - 1 roundings of a growing sum, and the fixture's own


def measure_restatements_triangulate(tri_groups, oracle):
    worst = {}
    for name, g in tri_groups.items():
        tin = gen.tri_input(g)
        for got in (oracle.triangulate(tin, g["depth_in"]),
                    np_ref.triangulate(tin.start_frame, tin.obs_offset, tin.obs_point, tin.Ps, tin.Rs, tin.tic, tin.ric, g["depth_in"], tin.init_depth)):
            worst[tri_regime(name)] = max(worst.get(tri_regime(name), 0.0), tri_check(name, got, g, np.inf))
    return worst


def test_restatements_triangulate(tri_groups, oracle):
    worst = measure_restatements_triangulate(tri_groups, oracle)
    print({k: f"{v:.3f}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= REF_TRI[k], (k, v)


def measure_restatements_shift(shift_cases, oracle):
    worst = {}
    for name, c in shift_cases.items():
        for got in (oracle.shift_depth(*gen.shift_args(c)),
                    np_ref.shift_depth(c["uv"], c["marg_R"], c["marg_P"], c["new_R"], c["new_P"], c["depth"], float(c["init_depth"]))):
            worst[name] = max(worst.get(name, 0.0), shift_check(name, got, c, np.inf))
    return worst


def test_restatements_shift_depth(shift_cases, oracle):
    worst = measure_restatements_shift(shift_cases, oracle)
    print({k: f"{v:.3f}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= REF_SHIFT[k], (k, v)


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pre_device(eng, pre_cases):
    """Every stored interval alone in a call of its own (noise vectors differ between cases)."""
    return [abi.preint_to_array(eng.preintegrate([c[4]], c[3])[0]) for c in pre_cases]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(PRE_IDS)), ids=PRE_IDS)
def test_gpu_preintegrate_vs_50_digits(pre_device, pre_cases, oracle, k):
    tag, regime, n, noise, (ba, bg, a0, g0, dts, accs, gyrs), ref = pre_cases[k]
    got = pre_device[k]
    worst = {}
    fold(worst, pre_metrics(got, ref))
    print(tag, {k: f"{v[0]:.2e}" + ("" if isinstance(v[1], str) else f" [{v[1][1]},{v[1][2]}]") for k, v in worst.items()})
    pre_structure(tag, got, noise)
    assert got[0] == oracle.preintegrate(a0, g0, ba, bg, dts, accs, gyrs, noise).sum_dt, f"{tag} sum_dt"
    assert np.array_equal(got[11:14], ba) and np.array_equal(got[14:17], bg), f"{tag} linearized biases"
    pre_check(tag, regime, got, ref)
    pre_cov_checks(tag, regime, got, ref)


@pytest.mark.gpu
def test_gpu_preintegrate_interval_is_independent_of_the_call(eng, pre_device, pre_cases):
    """All cases of one noise vector in one call, in stored and in reversed order: bit-identical to the interval alone
    (an interval must not depend on its neighbours, its offset into the packed samples, or its block index)."""
    for noise in {tuple(c[3]) for c in pre_cases}:
        idx = [k for k, c in enumerate(pre_cases) if tuple(c[3]) == noise]
        for order in (idx, idx[::-1]):
            got = eng.preintegrate([pre_cases[k][4] for k in order], list(noise))
            for k, g in zip(order, got):
                assert np.array_equal(abi.preint_to_array(g), pre_device[k]), f"{pre_cases[k][0]} at position {order.index(k)} of {len(order)}"
    # and the whole list at once: the intervals do not read the call's noise except through their covariance
    got = eng.preintegrate([c[4] for c in pre_cases], NOISE)
    for k, g in enumerate(got):
        a = abi.preint_to_array(g)
        assert np.array_equal(a[:242], pre_device[k][:242]), pre_cases[k][0]
        if tuple(pre_cases[k][3]) == tuple(NOISE):
            assert np.array_equal(a, pre_device[k]), pre_cases[k][0]


@pytest.mark.gpu
def test_gpu_preintegrate_600_ragged_intervals_vs_oracle(eng, oracle):
    """n drawn from 0 .. 70, usual regime, one call: per block against the oracle; bars widened by the oracle's own
    measured error against the 50-digit fixtures (the two errors add)."""
    rng = np.random.default_rng(20248)
    ivs = []
    for k in range(600):
        n = int(rng.integers(0, 71))
        ivs.append((rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3), rng.normal(0, 3, 3) + [0, 0, 9.8], rng.normal(0, 0.5, 3),
                    rng.uniform(0.002, 0.008, n), rng.normal(0, 3, (n, 3)) + [0, 0, 9.8], rng.normal(0, 0.5, (n, 3))))
    got = eng.preintegrate(ivs, NOISE)
    worst = {}
    for k, (ba, bg, a0, g0, dts, accs, gyrs) in enumerate(ivs):
        g, w = abi.preint_to_array(got[k]), abi.preint_to_array(oracle.preintegrate(a0, g0, ba, bg, dts, accs, gyrs, NOISE))
        tag = f"interval {k} (n = {len(dts)})"
        assert g[0] == w[0], f"{tag} sum_dt"
        if len(dts) == 0:
            assert np.array_equal(g, w), tag
            continue
        pre_structure(tag, g, NOISE)
        fold(worst, pre_check(tag, "usual", g, w, extra=REF_PRE["usual"]))
    print({k: f"{v[0]:.2e} {v[1]}" for k, v in worst.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRI_IDS)
def test_gpu_triangulate_vs_50_digits(eng, tri_groups, name):
    g = tri_groups[name]
    worst = tri_check(name, eng.triangulate(gen.tri_input(g), g["depth_in"]), g, bar(REF_TRI[tri_regime(name)], floor=2.0))
    print(f"{name}: worst {worst:.3f} eps sigma1/sigma4")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 5000])
def test_gpu_triangulate_sizes_vs_oracle(eng, oracle, N):
    w = synth.make_window(20 + N % 7, N)
    tin = abi.TriangulateIn(w)
    d0 = -np.ones(N)
    d0[::3] = 2.5
    got, want = eng.triangulate(tin, d0), oracle.triangulate(tin, d0)
    assert np.array_equal(got[::3], d0[::3])
    assert np.array_equal(got == tin.init_depth, want == tin.init_depth)
    m = tri_metric(got, want, tri_systems(tin))
    b = bar(REF_TRI["window"], floor=2.0) + REF_TRI["window"]
    print(f"N = {N}: worst {m.max():.3f} eps sigma1/sigma4 at landmark {m.argmax()}")
    bad = np.flatnonzero(~(m <= b))
    assert len(bad) == 0, "\n".join(f"N = {N} landmark {l}: {m[l]:.2f} > bar {b:.2f} [eps cond]" for l in bad[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIFT_IDS)
def test_gpu_shift_depth_vs_50_digits(eng, shift_cases, name):
    c = shift_cases[name]
    worst = shift_check(name, eng.shift_depth(*gen.shift_args(c)), c, bar(REF_SHIFT[name], floor=2.0))
    print(f"{name}: worst {worst:.3f} eps terms")


@pytest.mark.gpu
def test_gpu_feature_steps_between_begin_and_finish(pre_cases, tri_groups):
    """lfvio_triangulate and lfvio_preintegrate while the marginalization of a split optimization() call is in flight:
    the bits of an idle context, and finish() hands over the prior of the uninterrupted call."""
    from lfvio.engine import Engine
    from test_early_solution import same_prior, same_solution, serial, split, whole

    w = synth.make_window(0, 300)
    ref_sol, ref_prior = whole(serial(), w, abi.MARGIN_OLD)
    idle = Engine(0)
    g = tri_groups["w0_300"]
    ivs = [c[4] for c in pre_cases if c[1] == "usual"]
    idle_tri = idle.triangulate(gen.tri_input(g), g["depth_in"])
    idle_pre = [abi.preint_to_array(p) for p in idle.preintegrate(ivs, NOISE)]
    idle.close()
    eng = Engine(0)
    got = {}

    def between():
        got["tri"] = eng.triangulate(gen.tri_input(g), g["depth_in"])
        got["pre"] = [abi.preint_to_array(p) for p in eng.preintegrate(ivs, NOISE)]

    split(eng, w, abi.MARGIN_OLD)  # captures the graphs; the second call replays them
    sol, prior, _ = split(eng, w, abi.MARGIN_OLD, between)
    same_solution(sol, ref_sol)
    same_prior(prior, ref_prior)
    assert np.array_equal(got["tri"], idle_tri)
    assert len(got["pre"]) == len(idle_pre) and all(np.array_equal(a, b) for a, b in zip(got["pre"], idle_pre))
    eng.close()
