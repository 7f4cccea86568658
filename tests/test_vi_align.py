"""lfvio_vi_align (k_va_bias, k_va_align around two launches of k_preintegrate) against a 50-digit reference.

The fixtures tests/golden/vialign_hp.npz hold the regimes of tests/vialign_ref.py (REGIMES, FAILING) with the results of its
mpmath side rounded to double; `python tests/vialign_ref.py` writes them.  Metrics, each in the unit its error scales with
(vialign_ref.units / errors):

  delta_bg                  |difference| in units of eps * kappa(A_3) * |delta_bg|           (the 3 x 3 normal matrix)
  g_linear, s_linear        in units of eps * kappa(A) * |x| of LinearAlignment's system      (x: the whole solution, scale entry as solved)
  g_iter[k]                 the same of the system RefineGravity's iteration k factors
  g, s, x                   the same of the last one; x = the 3F velocities
  pre                       the re-propagated pre-integrations, per 3 x 3 block relative to the block (as test_feature_hp.py),
                            in the regimes whose 50-digit pre-integrations are stored (vialign_ref.KEEP_PRE)

BARS.  bar = 16 x the error the numpy restatement (vialign_ref.align_np, pivoted LDL^T) makes against the same fixture in the same
unit, per metric and regime; the generator stores that error beside the fixture and test_restatement_holds_its_record
re-measures it.  No floor.  kappa is large here (the scale column is badly scaled against the velocities, 1e4 .. 1e10), so both
sides sit far below one unit.

restatement / bar / device (MI355X), in the units above (pre: relative to the block); g_iter1, g_iter2 lie between g_iter0 and
g_iter3, g equals g_iter3
  regime           delta_bg                   g_linear                   s_linear                   g_iter0                    g_iter3                    s                          x                          pre
  f11_clean        15/2.5e+02/12              1.1e-06/1.7e-05/4.4e-06    8.8e-05/0.0014/0.00046     2.5e-07/4e-06/1.8e-06      8.6e-06/0.00014/5.6e-07    0.00052/0.0083/0.00031     4.1e-05/0.00066/2.5e-05    -
  f4_long          5.5e+05/8.8e+06/5.4e+05    1.3e-05/0.00021/1.5e-05    0.00047/0.0075/0.00059     4.5e-06/7.2e-05/3.3e-06    4.1e-05/0.00066/6.3e-05    0.0004/0.0064/0.00046      2.4e-05/0.00038/2.4e-05    4.9e-15/7.9e-14/2.7e-15
  f5_mixed         2.4e+05/3.9e+06/1e+05      0.028/0.45/0.017           0.073/1.2/0.045            0.0096/0.15/0.014          5.5/88/3.4                 0.036/0.58/0.075           0.023/0.37/0.047           6.3e-15/1e-13/3.3e-15
  f11_noisy        3.4/55/3.9                 2e-07/3.3e-06/1.6e-07      1.7e-05/0.00028/1.4e-05    4.8e-08/7.7e-07/1.9e-07    1.3e-06/2.1e-05/3.1e-07    1e-05/0.00017/3e-05        1.6e-07/2.6e-06/4.7e-07    -
  f30_fast         2/32/1.6                   2.9e-10/4.7e-09/7.1e-10    3.1e-07/5e-06/7.6e-07      4.1e-10/6.6e-09/9.4e-10    6.8e-10/1.1e-08/8.4e-10    6.4e-07/1e-05/1.2e-06      1.9e-09/3e-08/3.4e-09      -
  f30_translation  2/31/1.6                   1.1e-05/0.00017/5.6e-06    0.00046/0.0074/0.00023     9e-06/0.00014/2.4e-06      8.6e-06/0.00014/5.6e-06    6.8e-05/0.0011/0.00029     1.6e-05/0.00026/4.1e-05    -
  f30_rotation     9.2e+04/1.5e+06/9.6e+04    5.6e-08/9e-07/1.6e-08      2.6e-05/0.00042/7.5e-06    8e-09/1.3e-07/7.2e-09      2.4e-07/3.9e-06/1e-07      2.6e-06/4.1e-05/1.9e-06    2.5e-08/4e-07/2.2e-08      -
  f11_down         3.5/56/2.5                 1.2e-05/0.00019/7.5e-06    0.00042/0.0067/0.00026     1.3e-05/0.0002/8e-06       2.1e-05/0.00034/2.5e-05    0.00047/0.0075/0.00048     3.9e-05/0.00062/4e-05      -
  f11_up           0/0/0                      3.4e-06/5.5e-05/3.2e-06    0.00024/0.0038/0.00022     0/0/0                      0/0/0                      0.00026/0.0041/0.00021     9.6e-06/0.00015/7.7e-06    -
  f128_noisy       4.5/72/5.7                 0.00052/0.0083/0.00049     0.017/0.28/0.018           0.00049/0.0078/0.00045     0.00036/0.0057/0.00054     0.0069/0.11/0.012          0.0071/0.11/0.009          -
  (f11_up: nothing rotates and everything moves along z, so delta_bg and the x, y of every g0 are exact zeros on all three sides.)

status is exact in every regime.  RefineGravity's accumulation (A, b cleared once, :61-64, scaled inside the loop, :111-112) is
checked on g_iter[3]: the device is within the bar of the literal 50-digit value and further than the bar from what the
restatement gives when it clears A and b per iteration, in every regime where the two differ by >= 100 bars.
"""
import ctypes as C
import os

import numpy as np
import pytest

import vialign_ref as va

FACTOR = 16.0


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return va.load(os.path.join(golden_dir, "vialign_hp.npz"))


def call(eng, r, **kw):
    return eng.vi_align(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"], **kw)


def pre_arrays(res, F):
    from lfvio import abi

    return [None] + [abi.preint_to_array(res["pre"][k]) for k in range(1, F)]


PARITY = [n for n in va.REGIMES]


def test_fixture_file_covers_the_regimes(fixtures):
    """CPU: the file holds every regime of the generator, within the size of the other *_hp.npz files; the regimes span
    F = 4 .. 128, span lengths 1 .. 200, and every status."""
    assert set(fixtures) == set(va.REGIMES) | set(va.FAILING)
    assert os.path.getsize(va.GOLDEN) <= 350 * 1024
    assert sorted({len(fixtures[n]["R"]) for n in PARITY}) == [4, 5, 11, 30, 128]
    lengths = set()
    for n in PARITY:
        lengths |= {len(s[4]) for s in fixtures[n]["spans"][1:]}
    assert {1, 7, 20, 200} <= lengths
    assert sorted({fixtures[n]["hp"]["status"] for n in fixtures}) == [0, 1, 2, 3]


def test_restatement_holds_its_record(fixtures):
    """CPU: the numpy restatement against the 50-digit fixtures makes the errors the file records (the bars are 16 x those),
    its status is the fixture's in every regime, and its s and g are within 1e-6 relative of the 50-digit ones."""
    for name in PARITY:
        r = fixtures[name]
        ref = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"])
        assert ref["status"] == r["hp"]["status"] == 0, name
        assert abs(ref["s"] - r["hp"]["s"]) <= 1e-6 * abs(r["hp"]["s"]) and np.linalg.norm(ref["g"] - r["hp"]["g"]) <= 1e-6 * r["G"], name
        err = va.errors(ref, r["hp"], r["unit"])
        for m in va.METRICS:
            assert err[m] <= 2.0 * r["np_err"][m] + 1e-300, (name, m, err[m], r["np_err"][m])  # (2 x: another BLAS may round a product differently)
    for name in va.FAILING:
        r = fixtures[name]
        ref = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"])
        if r["hp"]["status"] != 3:  # (the pivoted factorization goes on where the device's reports a zero pivot)
            assert ref["status"] == r["hp"]["status"], name


def test_tangent_basis_branch_is_taken(fixtures):
    """CPU: the upright regime leaves g along +z exactly, so TangentBasis compares equal (:43) in every iteration."""
    r = fixtures["f11_up"]
    ref = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"])
    assert np.all(ref["g_linear"][:2] == 0) and np.all(ref["g_iter"][:, :2] == 0) and np.all(ref["g_iter"][:, 2] == r["G"])
    assert np.array_equal(va.tangent_basis_np(ref["g"]), np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]))


@pytest.mark.gpu
def test_fixtures_every_metric_per_regime(eng, fixtures):
    """Every metric on every parity regime, the device held to 16 x the restatement's own error; status exact."""
    bad, rows = [], []
    for name in PARITY:
        r = fixtures[name]
        F = len(r["R"])
        d = call(eng, r, with_pre=True)
        assert d["rc"] == 0 and d["status"] == 0, (name, d["status"])
        err = va.errors(d, r["hp"], r["unit"])
        for m in va.METRICS:
            bar = FACTOR * r["np_err"][m]
            rows.append(f"  {name:16s} {m:9s} {r['np_err'][m]:10.3g} / {bar:10.3g} / {err[m]:10.3g}")
            if not err[m] <= bar:
                bad.append(rows[-1])
        pa = pre_arrays(d, F)
        for k in range(1, F):  # the bias the spans were integrated again with is the one reported
            bg = np.asarray(r["spans"][1][1]) + d["delta_bg"]
            assert np.array_equal(pa[k][11:14], np.zeros(3)) and np.array_equal(pa[k][14:17], bg), (name, k)
        if "pre" in r["hp"]:
            e = max(va.pre_block_errors(pa[k], r["hp"]["pre"][k]) for k in range(1, F))
            bar = FACTOR * r["pre_np_err"]
            rows.append(f"  {name:16s} {'pre':9s} {r['pre_np_err']:10.3g} / {bar:10.3g} / {e:10.3g}")
            if not e <= bar:
                bad.append(rows[-1])
    print("regime, metric: restatement / bar / device")
    print("\n".join(rows))
    assert not bad, "over the bar:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_refine_gravity_accumulates(eng, fixtures):
    """g_iter shows that A and b are cleared once: the device is on the literal side of the variant that clears them per
    iteration, by more than the bar, wherever the two are >= 100 bars apart (the generator asserts such a regime exists)."""
    seen = 0
    for name in PARITY:
        r = fixtures[name]
        zeroed = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"], zero_per_iteration=True)
        bar = FACTOR * r["np_err"]["g_iter3"] * r["unit"]["g_iter3"]
        gap = np.linalg.norm(zeroed["g_iter"][3] - r["hp"]["g_iter"][3])
        if gap == 0 or gap < 100 * bar:
            continue
        seen += 1
        d = call(eng, r)
        lit, var = np.linalg.norm(d["g_iter"][3] - r["hp"]["g_iter"][3]), np.linalg.norm(d["g_iter"][3] - zeroed["g_iter"][3])
        print(f"{name}: variants {gap:.3g} apart, bar {bar:.3g}; device to the literal one {lit:.3g}, to the zeroed one {var:.3g}")
        assert lit <= bar < var, name
    assert seen >= 1


@pytest.mark.gpu
def test_tangent_basis_branch_on_the_device(eng, fixtures):
    """g along +z exactly: the comparison of :43 holds on the device too (x and y of every g0 are exact zeros)."""
    d = call(eng, fixtures["f11_up"])
    assert d["status"] == 0 and np.all(d["g_linear"][:2] == 0) and np.all(d["g_iter"][:, :2] == 0) and np.all(d["g_iter"][:, 2] == fixtures["f11_up"]["G"])


def marked_outputs(F):
    from lfvio import abi

    out = abi.ViAlignOutC()
    out.status = 77
    for k in range(3):
        out.delta_bg[k], out.g_linear[k], out.g[k] = 1.5 + k, 2.5 + k, 3.5 + k
        for j in range(4):
            out.g_iter[j][k] = 4.5 + 3 * j + k
    out.s_linear, out.s = 20.5, 21.5
    x = np.full(3 * F, 9.25)
    pre = (abi.Preintegration * F)()
    for k in range(F):
        pre[k].sum_dt = 5.0 + k
    return out, x, pre


@pytest.mark.gpu
def test_statuses_leave_outputs_alone(eng, fixtures):
    """status 1, 2 and 3: the status is the fixture's; x and pre stay as the caller had them, and with status 3 every field."""
    for name in va.FAILING:
        r = fixtures[name]
        F = len(r["R"])
        out, x, pre = marked_outputs(F)
        before_out, before_pre = bytes(out), bytes(pre)
        d = call(eng, r, out=out, x=x, pre=pre)
        assert d["rc"] == 0 and d["status"] == r["hp"]["status"], (name, d["status"], r["hp"]["status"])
        assert np.all(x == 9.25) and bytes(pre) == before_pre, name
        if d["status"] == 3:
            assert bytes(out)[8:] == before_out[8:], name
        else:  # what the reference had computed before the gate: delta_bg and the linear result (Bgs have moved by then)
            ref = va.align_np(r["R"], r["T"], r["spans"], r["noise"], r["tic"], r["G"])
            assert np.allclose(d["delta_bg"], ref["delta_bg"], rtol=1e-6, atol=1e-12) and np.isclose(d["s_linear"], ref["s_linear"], rtol=1e-6)


@pytest.mark.gpu
def test_argument_errors(eng, fixtures):
    """LFVIO_ERR_ARG with the outputs untouched: null pointers, F outside [4, 128], a span without samples, a span with sum_dt == 0."""
    from lfvio import abi

    r = fixtures["f11_clean"]
    F = len(r["R"])

    def refused(R, T, spans):
        out, x, pre = marked_outputs(max(len(spans), 1))
        b_out, b_pre = bytes(out), bytes(pre)
        d = eng.vi_align(R, T, spans, r["noise"], r["tic"], r["G"], out=out, x=x, pre=pre, check=False)
        assert d["rc"] == -1 and bytes(out) == b_out and bytes(pre) == b_pre and np.all(x == 9.25)

    refused(r["R"][:3], r["T"][:3], r["spans"][:3])
    big = [None] + [r["spans"][1]] * 128
    refused(np.tile(np.eye(3), (129, 1, 1)), np.zeros((129, 3)), big)
    empty = list(r["spans"])
    s = empty[4]
    empty[4] = (s[0], s[1], s[2], s[3], s[4][:0], s[5][:0], s[6][:0])
    refused(r["R"], r["T"], empty)
    still = list(r["spans"])
    still[7] = (s[0], s[1], s[2], s[3], np.zeros_like(s[4]), s[5], s[6])
    refused(r["R"], r["T"], still)
    out, x, _ = marked_outputs(F)
    b_out = bytes(out)
    vin = abi.ViAlignInC()
    vin.num_frames = F
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert eng.lib.lfvio_vi_align(eng.ctx, C.byref(vin), C.byref(out), xp, None) == -1  # null arrays
    assert eng.lib.lfvio_vi_align(eng.ctx, None, C.byref(out), xp, None) == -1
    assert eng.lib.lfvio_vi_align(eng.ctx, C.byref(vin), None, xp, None) == -1
    assert eng.lib.lfvio_vi_align(eng.ctx, C.byref(vin), C.byref(out), None, None) == -1
    assert bytes(out) == b_out and np.all(x == 9.25)
    d = call(eng, r)  # and the context goes on working
    assert d["status"] == 0


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("delta_bg", "g_linear", "g_iter", "g", "x")) and (a["status"], a["s_linear"], a["s"]) == (b["status"], b["s_linear"], b["s"])


@pytest.mark.gpu
def test_same_input_same_bits(eng, fixtures):
    """Two calls with the same input give the same bits (fixed summation order, no atomics), also after a call of another size."""
    for name in ("f11_noisy", "f128_noisy", "f5_mixed"):
        r = fixtures[name]
        a = call(eng, r, with_pre=True)
        call(eng, fixtures["f30_fast"])
        b = call(eng, r, with_pre=True)
        assert same_bits(a, b), name
        assert bytes(a["pre"])[ C.sizeof(a["pre"][0]):] == bytes(b["pre"])[C.sizeof(b["pre"][0]):], name


@pytest.mark.gpu
def test_beside_an_optimization_in_flight(eng, fixtures):
    """Between lfvio_batch_optimize_begin and _finish: the optimization's state and prior are the bits of the call without
    anything in between, and the alignment's result is the bits of a call on an idle context."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    w = synth.make_window(0, 300)
    r = fixtures["f30_fast"]
    alone = call(eng, r)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    def between(e):
        tin = abi.TriangulateIn(w)
        d0 = e.triangulate(tin, np.full(w.N, -1.0))
        res = call(e, r)
        d1 = e.triangulate(tin, np.full(w.N, -1.0))
        assert np.array_equal(d0, d1)
        return res

    sol0, prior0, _ = split(Engine(0), None)
    sol1, prior1, res = split(Engine(0), between)
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert same_bits(res, alone)
