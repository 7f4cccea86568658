"""CPU: the numpy restatement of the incremental part of GlobalSFM::construct (tests/sfm_chain_ref.py) against the 50-digit fixtures
tests/golden/sfm_chain_hp.npz, and the conditions of tests/golden/gen_sfm_chain_hp.py re-checked from the file."""
import os

import numpy as np
import pytest

import pnp_ref as pr
import sfm_chain_ref as cr
import test_sfm_chain as tc
from golden import gen_sfm_chain_hp as gen


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "sfm_chain_hp.npz"))
    return {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["names"]}


def test_restatement_holds_its_record(fixtures):
    """The restatement against the 50-digit fixtures is what test_sfm_chain.REF says (REF is rounded up to two digits), on every metric;
    its discrete results (tri_op, pnp_op, pnp_count, num_triangulated, status) equal the fixtures' (asserted by measure_restatement)."""
    got = tc.measure_restatement(fixtures)
    for r in tc.REGIMES:
        print(f'    "{r}": dict(' + ", ".join(f"{k}={v:.2g}" for k, v in got[r].items()) + "),")
    for r in tc.REGIMES:
        assert set(got[r]) == set(tc.REF[r]), r
        for k, v in got[r].items():
            assert v <= tc.REF[r][k] * (1 + 1e-9), (r, k, v, tc.REF[r][k])
            assert v >= 0.5 * tc.REF[r][k] or tc.REF[r][k] <= 1.0, f"REF[{r}][{k}] = {tc.REF[r][k]} is stale: measured {v}"


def test_schedule_numbers_the_ops_in_the_references_order():
    """3 F - 4 - l ops; the PnPs are the frames other than l and F - 1, forward ones ascending then backward ones descending; one closing op."""
    for F in range(2, 12):
        for l in range(F - 1):
            ops = cr.schedule(F, l)
            assert len(ops) == 3 * F - 4 - l and ops[-1][0] == "close" and [o[0] for o in ops].count("close") == 1
            assert [a for k, a, _ in ops if k == "pnp"] == list(range(l + 1, F - 1)) + list(range(l - 1, -1, -1))
            assert ops[0] == ("tri", l, F - 1)
    assert cr.schedule(4, 1) == [("tri", 1, 3), ("pnp", 2, 2), ("tri", 2, 3), ("tri", 1, 2), ("pnp", 0, 0), ("tri", 0, 1), ("close", 0, 0)]


def test_fixture_conditions(fixtures):
    """The file holds the scenes it is meant to, and the generator's conditions hold: stored from the 50-digit run, and re-measured here in
    double precision on the restatement (pin and gap >= 1.05, every PnP that ran has >= 10 correspondences, sv <= 0.2, no zero fourth entry)."""
    assert set(fixtures) == set(gen.CASES) | set(gen.STOPPED)
    shape = lambda c: (int(fixtures[c]["F"]), len(fixtures[c]["off"]) - 1, int(fixtures[c]["l"]))
    assert shape("f2_p6") == (2, 6, 0) and shape("f3_p12_l0") == (3, 12, 0) and shape("f3_p12_l1") == (3, 12, 1)
    assert [shape(c) for c in ("f11_l0", "f11_l5", "f11_l9")] == [shape(c + "_exact") for c in ("f11_l0", "f11_l5", "f11_l9")] == [(11, 60, 0), (11, 60, 5), (11, 60, 9)]
    assert shape("f4_p257") == (4, 257, 1) and shape("f4_p4096") == (4, 4096, 1) and shape("ragged") == (6, 37, 2) and shape("ragged_short") == (6, 36, 2)
    assert not np.any(fixtures["f2_p6"]["pnp_op"] >= 0)
    assert list(fixtures["f3_p12_l0"]["pnp_op"] >= 0) == [False, True, False] and list(fixtures["f3_p12_l1"]["pnp_op"] >= 0) == [True, False, False]
    for c in fixtures:
        z = fixtures[c]["bearing"][:, 2]
        assert np.any(z < -0.1) and np.any(z > 0.1), c
    rag = fixtures["ragged"]
    cnt, close = np.diff(rag["off"]), 3 * 6 - 4 - 2 - 1
    assert np.sum(cnt == 1) == 1 and rag["tri_op"][cnt == 1][0] == -1 and int(rag["num_triangulated"]) == 36
    only_close = np.nonzero(rag["tri_op"] == close)[0]
    assert sorted(tuple(rag["frame"][rag["off"][j]:rag["off"][j + 1]]) for j in only_close) == [(0, 1), (3, 4)]
    assert rag["pnp_count"][0] == 10 and fixtures["ragged_short"]["pnp_count"][0] == 9 and int(fixtures["ragged_short"]["status"]) == 1
    for c in gen.CASES:  # a closing op that triangulates something, on the 11-frame scenes with random tracks
        if shape(c)[0] == 11:
            assert np.any(fixtures[c]["tri_op"] == 3 * shape(c)[0] - 4 - shape(c)[2] - 1), c
    for c, f in fixtures.items():
        pin, gap, count, sv, w = f["cond"]
        assert pin >= gen.PIN_CAP and gap >= gen.GAP_CAP and count >= 10 and sv <= gen.SV_CAP and w > 0, (c, f["cond"])
        res = cr.construct(*tc.args_of(f))
        cd = gen.conditions(res, int(f["F"]), int(f["l"]))
        print(f"  {c:14s} " + " ".join(f"{k} {v:.4g}" for k, v in cd.items()))
        assert gen.conditions_hold(cd), (c, cd)


def test_fixtures_are_the_generators(fixtures):
    """The inputs of two cases re-made by the generator, bit for bit, and the 50-digit chain of the smallest one."""
    for name in ("f2_p6", "ragged_short"):
        sc = gen.make_scene(**{**gen.CASES, **gen.STOPPED}[name])
        for k in ("off", "frame", "bearing", "relative_R", "relative_T"):
            assert np.array_equal(sc[k], fixtures[name][k]), (name, k)
    f = fixtures["f2_p6"]
    h = cr.construct(*tc.args_of(f), pr.HP)
    assert np.array_equal(pr.to_double(h["position"]), f["position"]) and np.array_equal(pr.to_double(h["c_rotation"]), f["c_rotation"])


def test_a_pnp_gets_the_50_digit_positions_unrounded(fixtures):
    """The 50-digit chain hands compute_pose() its positions as they are: the backend that carries them returns them for their rounding."""
    pws = pr.HP.arr(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])) + pr.HP.mp.mpf(10) ** -30
    be = cr._HPCarry(pws)
    back = be.arr(pr.to_double(pws))
    assert all(a == b for a, b in zip(back.reshape(-1), pws.reshape(-1))) and back[0, 0] != pr.HP.num(1.0)
    assert be.arr(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 7.0]]))[1, 2] == pr.HP.num(7.0)


def test_stopped_chain_and_compaction(fixtures):
    """Status 1 at 9 correspondences leaves frame 0 unposed; compact() keeps the triangulated points, in order, with their observations."""
    f = fixtures["ragged_short"]
    res = cr.construct(*tc.args_of(f))
    assert res["status"] == 1 and res["failed_frame"] == 0 and list(res["posed"]) == [False, True, True, True, True, True]
    assert np.all(np.isnan(res["c_rotation"][0])) and 0 not in res["pnp"]
    f = fixtures["ragged"]
    res = cr.construct(*tc.args_of(f))
    cp = cr.compact(res, f["off"], f["frame"], f["bearing"])
    assert len(cp["keep"]) == 36 and cp["off"][-1] == len(cp["frame"]) == f["off"][-1] - 1 and np.array_equal(cp["position"], res["position"][cp["keep"]])
