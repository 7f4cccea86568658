"""lfvio_klt_track / lfvio_klt_reset / lfvio_klt_level (k_klt_down, k_klt_track) against the float64 numpy restatement
tests/klt_ref.py, through its fixture tests/golden/klt_cases.npz (tests/test_klt_ref.py holds the two equal bit for bit).  Images are
rendered from seeds (klt_ref.make_case); shapes (a)-(e) are the smallest that reach each path: odd sizes, a top level of 44 x 43
under a 41 window, the level rule cutting 3 levels to 1, a small window, the smallest image.

  1  lfvio_klt_level equals the restatement's levels exactly;
  2  status, levels_used, num_tracked equal the restatement's; next_pts within 0.02 px of it on every point it tracked in fewer than
     max_iterations iterations at every level (at most 5 % of the points may be excluded: the restatement excludes none).  The bar is
     the stopping rule's: two runs that stop one iteration apart differ by one step of at most 0.01 px plus what was left, which is
     less than that under contraction.  Measured: worst 1.5e-5 px, 0 of 740 points with other iteration counts, none excluded;
  3  the status cases of tests/test_klt_ref.py;
  4  a point's bits depend neither on N nor on its index nor on the run; N = 0 makes the image resident;
  5  residency: A, B, C on one context gives the bits of a fresh context given B, C; after lfvio_klt_reset and after another image
     size the image is tracked against itself: zero flow, one iteration per level;
  6  argument errors leave outputs and the resident image alone; the staging block regrows;
  7  beside an optimization in flight."""
import functools
import os

import numpy as np
import pytest

import klt_ref as k

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "klt_cases.npz")
SEEDS = (0, 1, 2, 3)
NO_POINTS = np.zeros((0, 2), np.float32)


@functools.lru_cache(maxsize=None)
def case(name, seed):
    return k.make_case(name, seed)


@functools.lru_cache(maxsize=None)
def status_case():
    return k.make_status_case()


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {key: z[key] for key in z.files}


def pair(eng, c, pts=None, **kw):
    """img0 made resident (N = 0), then the points tracked into img1."""
    eng.klt_reset()
    r0 = eng.klt_track(c["img0"], NO_POINTS, win_size=c["win"])
    assert (r0["rc"], r0["num_tracked"], r0["levels_used"]) == (0, 0, c["levels_used"])
    return eng.klt_track(c["img1"], c["pts"] if pts is None else pts, win_size=c["win"], **kw)


def same_bits(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in ("next", "status", "iterations")) and (a["levels_used"], a["num_tracked"]) == (b["levels_used"], b["num_tracked"])


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_levels_are_exact(eng, name):
    c = case(name, 0)
    eng.klt_reset()
    assert eng.klt_level(0, check=False) is None
    eng.klt_track(c["img0"], NO_POINTS, win_size=c["win"])
    want = k.pyramid(c["img0"], c["win"], 3)
    assert len(want) == c["levels_used"] + 1
    for L, lv in enumerate(want):
        assert np.array_equal(eng.klt_level(L), lv), (name, L)
    assert eng.klt_level(len(want), check=False) is None and eng.klt_level(-1, check=False) is None


@pytest.mark.parametrize("name", sorted(k.CASES))
def test_against_the_restatement(eng, name):
    fx = fixture()
    total = excluded = differ = 0
    worst = 0.0
    for seed in SEEDS:
        c, key = case(name, seed), f"{name}_{seed}"
        d = pair(eng, c)
        assert np.array_equal(fx[key + "_pts"], c["pts"])
        assert np.array_equal(d["status"], fx[key + "_status"]), key
        assert [d["levels_used"], d["num_tracked"]] == fx[key + "_counts"].tolist(), key
        ok = (fx[key + "_iterations"] < 30).all(axis=1)
        dist = np.hypot(*(d["next"].astype(np.float64) - fx[key + "_next"].astype(np.float64)).T)
        total, excluded = total + len(ok), excluded + int((~ok).sum())
        differ += int((d["iterations"] != fx[key + "_iterations"]).any(axis=1).sum())
        worst = max(worst, float(dist[ok].max()))
        print(f"{key}: worst distance to the restatement {dist[ok].max():.3e} px over {int(ok.sum())} points")
        assert dist[ok].max() <= 0.02, (key, dist[ok].max())
    print(f"case {name}: worst {worst:.3e} px, {differ} of {total} points with other iteration counts, {excluded} excluded")
    assert excluded <= 0.05 * total


def test_status_cases(eng):
    fx, c = fixture(), status_case()
    for border, key in ((1, "status_b1"), (-1, "status_bm1")):
        d = pair(eng, c, border=border)
        assert np.array_equal(d["status"], fx[key + "_status"]), (border, d["status"])
        assert [d["levels_used"], d["num_tracked"]] == fx[key + "_counts"].tolist()
        assert np.array_equal(d["iterations"] > 0, fx[key + "_iterations"] > 0)  # the same levels skipped
    assert np.array_equal(fx["status_b1_status"], k.STATUS_WANT)


def test_independence_and_repeatability(eng):
    c = case("a", 0)
    N = len(c["pts"])
    assert N == 65

    def sequence():
        whole = pair(eng, c)
        rev = pair(eng, c, pts=c["pts"][::-1].copy())
        alone = [pair(eng, c, pts=c["pts"][n:n + 1]) for n in range(N)]
        return whole, rev, alone

    whole, rev, alone = sequence()
    assert whole["num_tracked"] == N
    for f in ("next", "status", "iterations"):
        assert rev[f][::-1].tobytes() == whole[f].tobytes(), f
        assert np.concatenate([a[f] for a in alone]).tobytes() == whole[f].tobytes(), f
    whole2, rev2, alone2 = sequence()
    assert same_bits(whole, whole2) and same_bits(rev, rev2) and all(same_bits(a, b) for a, b in zip(alone, alone2))
    # N = 0: LFVIO_OK, and the image is resident (pair() relies on it: here it is looked at)
    eng.klt_reset()
    r = eng.klt_track(c["img0"], NO_POINTS, want_iterations=False)
    assert (r["rc"], r["levels_used"], r["num_tracked"], len(r["next"])) == (0, 3, 0, 0)
    assert np.array_equal(eng.klt_level(0), c["img0"])
    assert same_bits(eng.klt_track(c["img1"], c["pts"]), whole)
    # without the iteration counts (a NULL pointer): the same points and status
    bare = pair(eng, c, want_iterations=False)
    assert bare["iterations"] is None and bare["next"].tobytes() == whole["next"].tobytes() and bare["status"].tobytes() == whole["status"].tobytes()


def self_tracked(d, pts, levels_used):
    return (np.array_equal(d["next"], pts) and np.all(d["status"] == 1) and np.all(d["iterations"][:, :levels_used + 1] == 1)
            and np.all(d["iterations"][:, levels_used + 1:] == 0) and d["levels_used"] == levels_used)


def test_residency(eng):
    from lfvio.engine import Engine

    c, c2 = case("a", 0), case("a", 1)
    A, B, C_ = c["img0"], c["img1"], c2["img1"]  # (C is another texture: what B -> C finds does not matter, only that both contexts find the same)
    eng.klt_reset()
    eng.klt_track(A, NO_POINTS)
    ab = eng.klt_track(B, c["pts"])
    bc = eng.klt_track(C_, ab["next"])
    fresh = Engine(0)
    try:
        b0 = fresh.klt_track(B, ab["next"])  # no resident image: B against itself
        assert self_tracked(b0, ab["next"], 3)
        assert same_bits(fresh.klt_track(C_, ab["next"]), bc)
    finally:
        fresh.close()
    assert np.array_equal(eng.klt_level(0), C_)
    eng.klt_reset()
    assert self_tracked(eng.klt_track(B, c["pts"]), c["pts"], 3)
    small = case("e", 0)
    assert self_tracked(eng.klt_track(small["img0"], small["pts"], win_size=small["win"]), small["pts"], 1)  # another size: against itself
    assert same_bits(eng.klt_track(small["img1"], small["pts"], win_size=small["win"]), pair(eng, small))
    # a call that asks for more levels than the resident pyramid was built with gets them built
    eng.klt_reset()
    eng.klt_track(A, NO_POINTS, max_level=1)
    assert eng.klt_level(2, check=False) is None
    assert same_bits(eng.klt_track(B, c["pts"]), ab)


REFUSED = [dict(size=(15, 339)), dict(size=(8193, 339)), dict(size=(345, 15)), dict(size=(345, 8193)), dict(num_points=-1), dict(num_points=4097),
           dict(win_size=3), dict(win_size=40), dict(win_size=43), dict(max_level=-1), dict(max_level=6), dict(max_iterations=0), dict(max_iterations=101),
           dict(epsilon=0.0), dict(epsilon=-0.01), dict(epsilon=float("nan")), dict(min_eig_threshold=-1e-9), dict(min_eig_threshold=float("nan"))]


def test_argument_errors_and_regrowth(eng):
    import ctypes as C

    from lfvio import abi

    c = case("a", 0)
    want = pair(eng, c)
    eng.klt_reset()
    eng.klt_track(c["img0"], NO_POINTS)
    nxt, stat = np.full((4097, 2), 7.5, np.float32), np.full(4097, 9, np.uint8)
    for over in REFUSED:
        d = eng.klt_track(c["img1"], c["pts"], next=nxt, status=stat, check=False, **over)
        assert d["rc"] == -1 and (d["levels_used"], d["num_tracked"]) == (-1, -1), over  # LFVIO_ERR_ARG, LfvioKltOut as it was
    for img, pts, n in ((None, c["pts"], None), (c["img1"], None, 5)):
        d = eng.klt_track(img, pts, next=nxt, status=stat, size=(345, 339), num_points=n, check=False)
        assert d["rc"] == -1 and (d["levels_used"], d["num_tracked"]) == (-1, -1)
    kin, out = abi.KltInC(), abi.KltOutC(-1, -1)
    fp, up = nxt.ctypes.data_as(C.POINTER(C.c_float)), stat.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert eng.lib.lfvio_klt_track(eng.ctx, None, fp, up, None, C.byref(out)) == -1
    assert eng.lib.lfvio_klt_track(eng.ctx, C.byref(kin), fp, up, None, C.byref(out)) == -1
    assert np.all(nxt == 7.5) and np.all(stat == 9)
    assert np.array_equal(eng.klt_level(0), c["img0"])  # the resident image is the one from before the refused calls ...
    assert same_bits(eng.klt_track(c["img1"], c["pts"]), want)  # ... and the next call tracks from it
    # a 1280 x 960 call regrows the staging block; the small case afterwards gives the same bits
    big = np.random.default_rng(5).integers(0, 256, (960, 1280)).astype(np.uint8)
    pts = np.random.default_rng(6).uniform(30, 900, (200, 2)).astype(np.float32)
    d = eng.klt_track(big, pts)
    assert d["rc"] == 0 and d["levels_used"] == 3 and self_tracked(d, pts, 3)
    assert np.array_equal(eng.klt_level(3), k.pyramid(big, 41, 3)[3])
    assert same_bits(pair(eng, c), want)


def test_beside_an_optimization_in_flight(eng):
    """Between lfvio_batch_optimize_begin and _finish: the optimization's state and prior are the bits of the call without anything in
    between, and the tracking result is the bits of a call on an idle context."""
    from lfvio import abi, synth
    from lfvio.engine import Engine

    w = synth.make_window(0, 300)
    c = case("a", 0)
    alone = pair(eng, c)

    def split(e, between):
        e.batch_reserve(1, w.N, w.M)
        e.batch_upload(0, w)
        sol = e.optimize_begin(abi.MARGIN_OLD, w.N)
        res = between(e) if between else None
        return sol, e.optimize_finish(), res

    e0, e1 = Engine(0), Engine(0)
    try:
        sol0, prior0, _ = split(e0, None)
        sol1, prior1, got = split(e1, lambda e: pair(e, c))
    finally:
        e0.close()
        e1.close()
    assert bytes(sol0.c.para_pose) == bytes(sol1.c.para_pose) and bytes(sol0.c.para_speed_bias) == bytes(sol1.c.para_speed_bias)
    assert bytes(sol0.c.para_ex_pose) == bytes(sol1.c.para_ex_pose) and sol0.c.para_td == sol1.c.para_td and np.array_equal(sol0.lam, sol1.lam)
    assert (prior0.valid, prior0.n, prior0.m) == (prior1.valid, prior1.n, prior1.m)
    assert np.array_equal(prior0.J(), prior1.J()) and np.array_equal(prior0.r(), prior1.r())
    assert same_bits(got, alone)
