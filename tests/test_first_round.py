"""The kernels' first round of loads, addressed from kernel arguments (-m gpu; csrc/slot_args.h).

k_lin and k_spec_begin take the offsets of the arrays they read first as an argument (SlotArgs, built from the context's Layout) and issue those loads with the slot header's, indices clamped to the arrays' CAPACITY — before
the header has said how large the window is.  Nothing of the arithmetic changes, so wherever a window is solved — in a context far larger
than it, behind a re-allocation, beside other windows, with or without captured graphs, worker streams or the 8-lane landmark role, from
a start point off the unit sphere — the solution (state, inverse depths, summary, trace) and the prior (J, r, blocks, linearization
points) are the SAME BYTES as in a fresh context reserved for exactly that window.  Shapes: the smallest that can go wrong — 0, 1, 24
and 33 landmarks (none, one lane, under and over half a landmark block) under a capacity of 320 (SPEC_MAX_LM: the largest that keeps
the route these kernels are on)."""
import os

import numpy as np
import pytest

from lfvio import abi, synth
from lfvio.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAGS = (abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW)
CAP_N, CAP_M = 320, 320 * 11


def golden(name):
    d = np.load(os.path.join(GOLDEN, name))
    return abi.window_from_dict({k[4:]: d[k] for k in d.files if k.startswith("win_")})


def no_landmarks(seed):
    w = synth.make_window(seed, 1)
    return w.copy(start_frame=np.zeros(0, np.int32), obs_offset=np.zeros(1, np.int32), inv_depth=np.zeros(0), obs_point=np.zeros((0, 3)),
                  obs_velocity=np.zeros((0, 3)), obs_cur_td=np.zeros(0), obs_uv_y=np.zeros(0))


def windows():
    return {"n24_prior": golden("window_n24_prior.npz"), "n24_notd_noex": golden("window_n24_notd_noex.npz"), "n0": no_landmarks(3),
            "n1": synth.make_window(4, 1), "n33": synth.make_window(5, 33)}


def solve(eng, w, flag, reserve=None):
    n, m = reserve if reserve is not None else (w.N, w.M)
    eng.batch_reserve(1, n, m)
    eng.batch_upload(0, w)
    eng.batch_optimize(1, flag)
    return eng.batch_download(0, w.N)


def fresh(w, flag, **switches):
    """a fresh context reserved for exactly this window"""
    eng = Engine(0)
    for key, on in switches.items():
        eng.configure(key, on)
    out = solve(eng, w, flag)
    eng.close()
    return out


def same(got, want):
    (a, p), (b, q) = got, want
    assert np.array_equal(a.pose, b.pose) and np.array_equal(a.speed_bias, b.speed_bias) and np.array_equal(a.ex_pose, b.ex_pose)
    assert bytes(a.c.para_pose) == bytes(b.c.para_pose) and bytes(a.c.para_speed_bias) == bytes(b.c.para_speed_bias)
    assert bytes(a.c.para_ex_pose) == bytes(b.c.para_ex_pose) and np.array_equal(np.float64(a.c.para_td), np.float64(b.c.para_td))
    assert np.array_equal(a.lam, b.lam)
    for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination", "initial_cost", "final_cost"):
        assert getattr(a.c, k) == getattr(b.c, k), k
    assert bytes(a.c.trace) == bytes(b.c.trace)
    assert (p.valid, p.n, p.m, p.num_blocks) == (q.valid, q.n, q.m, q.num_blocks) and p.block_list() == q.block_list()
    if p.valid:
        assert np.array_equal(p.J(), q.J()) and np.array_equal(p.r(), q.r())
        for i in range(p.num_blocks):
            assert np.array_equal(p.x0(i), q.x0(i)), i


@pytest.fixture(scope="module")
def exact():
    """every window solved in a fresh context reserved for exactly that window: (name, flag) -> (solution, prior).  Computed once."""
    ref = {}
    ws = windows()
    ws["n300"] = synth.make_window(0, 300)
    for k in (24, 40, 120):
        ws[f"batch{k}"] = synth.make_window(20 + k, k)
    for name, w in ws.items():
        for flag in FLAGS:
            ref[name, flag] = fresh(w, flag)
    return ws, ref


@pytest.mark.parametrize("name", ["n24_prior", "n24_notd_noex", "n0", "n1", "n33"])
def test_capacity_larger_than_the_window(exact, name):
    ws, ref = exact
    eng = Engine(0)
    for flag in FLAGS:
        for rep in range(2):  # (the second call replays the graphs the first one captured)
            same(solve(eng, ws[name], flag, reserve=(CAP_N, CAP_M)), ref[name, flag])
    eng.close()


def test_re_reserve(exact):
    """The arguments are baked into the captured graphs: a reserve() that changes the Layout has to drop them."""
    ws, ref = exact
    eng = Engine(0)
    flag = abi.MARGIN_OLD
    same(solve(eng, ws["n24_prior"], flag), ref["n24_prior", flag])
    same(solve(eng, ws["n300"], flag, reserve=(300, ws["n300"].M)), ref["n300", flag])
    same(solve(eng, ws["n24_prior"], flag), ref["n24_prior", flag])
    same(solve(eng, ws["n1"], flag), ref["n1", flag])
    eng.close()


def test_batch_of_three(exact):
    ws, ref = exact
    trio = [ws[f"batch{k}"] for k in (24, 40, 120)]
    eng = Engine(0)
    eng.batch_reserve(3, max(w.N for w in trio), max(w.M for w in trio))
    for flag in FLAGS:
        for s, w in enumerate(trio):
            eng.batch_upload(s, w)
        eng.batch_optimize(3, flag)
        for s, (k, w) in enumerate(zip((24, 40, 120), trio)):
            same(eng.batch_download(s, w.N), ref[f"batch{k}", flag])
    eng.close()


@pytest.mark.parametrize("key", ["graph", "marg_ahead", "lm_half"])
def test_switches(exact, key):
    """Same window, captured graphs / worker streams / the 8-lane landmark role on and off: under the large capacity the same bytes as
    with the same switch in a context of the window's size.  (The 4-lane landmark role adds a track's terms in another order than the
    8-lane one: its reference is its own.  Worker streams on or off are the same bytes by tests/test_marg_ahead.py: checked here too.)"""
    ws, ref = exact
    for name in ("n24_prior", "n33"):
        for on in (0, 1):
            eng = Engine(0)
            eng.configure(key, on)
            for flag in FLAGS:
                got = solve(eng, ws[name], flag, reserve=(CAP_N, CAP_M))
                same(got, fresh(ws[name], flag, **{key: on}))
                if key == "marg_ahead" or on == 1:
                    same(got, ref[name, flag])
            eng.close()


def test_off_sphere_start():
    """A start quaternion off the unit sphere: the first pass runs the <OFFS = true> instantiations."""
    w = synth.make_window(6, 24)
    w = w.copy()
    w.pose[10, 3:] *= 1.0 + 1e-8
    for flag in FLAGS:
        want = fresh(w, flag)
        eng = Engine(0)
        for rep in range(2):
            same(solve(eng, w, flag, reserve=(CAP_N, CAP_M)), want)
        eng.close()
