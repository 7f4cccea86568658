"""The debug hooks that run a pass and read a slot share one launch and one copy path (csrc/debug.inc): lfvio_debug_linearize is
lfvio_debug_pass_io on a freshly uploaded window with the role sweep forced and the landmarks back in the caller's order, and
Engine.resident_pass is a view on Engine.pass_io.  Both are held to pass_io here, bit for bit: the same kernels run on the same
uploaded state, so nothing but the host's copying can tell them apart.
"""
import numpy as np
import pytest

import lin_cases as lc
from test_lin_hp import assembled_of

pytestmark = pytest.mark.gpu

ROLES = 0  # lfvio_debug_query "sweep_kernel"
RESIDENT_KEYS = ("gp", "schur", "a", "b", "gn_p", "q")


def upload_all(eng, ws):
    eng.batch_reserve(len(ws), max(max(w.N for w in ws), 1), max(max(w.M for w in ws), 1))
    for s, w in enumerate(ws):
        eng.batch_upload(s, w)


@pytest.mark.parametrize("half", [1, 0], ids=["lanes8", "lanes4"])
@pytest.mark.parametrize("name", ["n1", "n65", "prior_old"])
def test_linearize_agrees_with_pass_io(eng, oracle, name, half):
    w = lc.window(oracle, name)
    try:
        eng.set_linw(0)
        eng.set_lm_half(half)
        lin = eng.linearize(w)
        upload_all(eng, [w])
        io = eng.pass_io(1, 0, w.N)
    finally:
        eng.set_linw(1)
        eng.set_lm_half(1)
    assert io["linw"] == ROLES
    got, order = assembled_of(io, w), lc.device_order(w)
    # (assembled_of mirrors the triangle by an addition, which would turn a -0.0 into 0.0: for the bits, the entries are placed instead)
    i, j = np.tril_indices(lin["H"].shape[0])
    H = np.zeros_like(lin["H"])
    H[i, j] = H[j, i] = io["H"]
    assert np.array_equal(H, got["H"]) and lin["H"].tobytes() == H.tobytes()
    assert lin["g"].tobytes() == np.asarray(got["g"]).tobytes()
    for k in ("a", "b", "W"):
        assert np.ascontiguousarray(lin[k][order]).tobytes() == np.ascontiguousarray(got[k]).tobytes(), k
    assert lin["cost"] == got["cost"]


def assert_view(rp, io):
    assert set(rp) == set(RESIDENT_KEYS) | {"lm_sum", "x_cost", "linw"}
    for k in RESIDENT_KEYS:
        assert rp[k].tobytes() == io[k].tobytes(), k
    assert rp["lm_sum"].shape == (5,) and rp["lm_sum"].tobytes() == io["lm_sum"][:5].tobytes()
    assert rp["x_cost"].shape == (1,) and rp["x_cost"][0] == io["x_cost"]
    assert rp["linw"] == io["linw"]


@pytest.mark.parametrize("names,linw,slot", [(("n65",), 2, 0), (("n65", "prior_old"), 0, 1)], ids=["one-linw2", "two-linw0-slot1"])
def test_resident_pass_agrees_with_pass_io(eng, oracle, names, linw, slot):
    ws = [lc.window(oracle, n) for n in names]
    try:
        eng.set_linw(linw)
        upload_all(eng, ws)
        rp = eng.resident_pass(len(ws), slot, ws[slot].N)
        io = eng.pass_io(len(ws), slot, ws[slot].N)
    finally:
        eng.set_linw(1)
    assert io["linw"] == (1 if linw == 2 else ROLES)
    assert_view(rp, io)
