"""The memory a context owns (lf-vio_amd/csrc/dev_mem.h; tests/test_dev_mem.py walks the rule itself on the CPU), seen from outside:
what growth, reuse and teardown must not change.  Every comparison is byte for byte against a fresh context; nothing is asserted about
free device memory (other processes share the card).  The shapes are klt_ref's smallest image (e, 97 x 75) and its 345 x 339 case (a):
going from one to the other grows the pyramid buffers, the detector's work arrays, the base mask and the staging block of the
feature stream, and coming back reuses them.

  1  small, large, small on ONE context with CLAHE on and a base mask set at each size: klt_track, gft_detect, gft_response,
     clahe_apply and a triangulate of the small golden window (the staging block is shared) give at every step the bytes of a fresh
     context that is handed only that step;
  2  create, use, destroy, create again: two rounds of the large step in one process give the same bytes, and close() returns;
  3  the base mask across a size change: a mask of the small size, the large image made resident: detection is refused; a mask of
     the large size: the fresh context's bytes."""
import functools
import os

import numpy as np
import pytest

import gft_ref as g
import klt_ref as k
from lfvio import abi
from lfvio.engine import Engine

pytestmark = pytest.mark.gpu
NO_POINTS = np.zeros((0, 2), np.float32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL, LARGE = "e", "a"
CLAHE = (3.0, (8, 8))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(klt case, base mask, tracked points and their counts) of one image size, computed once and read-only."""
    c = k.make_case(name, 0)
    h, w = c["img0"].shape
    mask = g.annulus_mask(w, h, w // 2, h // 2, int(0.47 * min(w, h)), min(w, h) // 16)
    pts, cnt = g.tracked_case(w, h, 0)
    for a in (c["img0"], c["img1"], c["pts"], mask, pts, cnt):
        a.setflags(write=False)
    assert (mask == 0).any() and (mask == 255).any()
    return c, mask, pts, cnt


@functools.lru_cache(maxsize=None)
def golden_window():
    d = np.load(os.path.join(GOLDEN, "window_n24.npz"))
    return abi.window_from_dict({key[4:]: d[key] for key in d.files if key.startswith("win_")})


def resident(e, name):
    c = inputs(name)[0]
    r = e.klt_track(c["img0"], NO_POINTS, win_size=c["win"])
    assert (r["rc"], r["levels_used"]) == (0, c["levels_used"])


def step(e, name):
    """Every call that owns or shares memory, at one image size; the outputs as a list of (what, bytes)."""
    c, mask, pts, cnt = inputs(name)
    resident(e, name)    # (first: a base mask is accepted only at the resident image's size)
    e.gft_set_mask(mask)
    t = e.klt_track(c["img1"], c["pts"], win_size=c["win"])
    assert t["num_tracked"] > 0
    out = [("klt " + f, t[f].tobytes()) for f in ("next", "status", "iterations")] + [("klt counts", (t["levels_used"], t["num_tracked"]))]
    out += [(f"level {lv}", e.klt_level(lv).tobytes()) for lv in range(t["levels_used"] + 1)]
    d = e.gft_detect(pts, cnt, min_distance=10, mask_radius=10)
    assert d["rc"] == 0 and len(d["corners"]) > 0 and 0 < len(d["kept"]) < len(pts)
    out += [("gft kept", d["kept"].tobytes()), ("gft corners", d["corners"].tobytes()), ("gft counts", (d["num_candidates"], np.float64(d["max_response"]).tobytes()))]
    out.append(("response", e.gft_response().tobytes()))
    eq, lut = e.clahe_apply(c["img0"], 2.0, (3, 5), want_lut=True)  # (another configuration than the setting's)
    out += [("clahe image", eq.tobytes()), ("clahe lut", lut.tobytes())]
    w = golden_window()
    depth = e.triangulate(abi.TriangulateIn(w), np.full(w.N, -1.0))
    assert (depth > 0).any()
    out.append(("triangulate", depth.tobytes()))
    return out


def fresh_step(name):
    e = Engine(0)
    try:
        e.clahe_set(*CLAHE)
        return step(e, name)
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def fresh(name):
    """... of a context that has seen nothing else: computed once, shared by the tests."""
    return fresh_step(name)


def assert_same(got, want, tag):
    assert [n for n, _ in got] == [n for n, _ in want], tag
    for (what, a), (_, b) in zip(got, want):
        assert a == b, (tag, what)


def test_growth_and_reuse_give_a_fresh_contexts_bits():
    e = Engine(0)
    try:
        e.clahe_set(*CLAHE)
        for n, name in enumerate((SMALL, LARGE, SMALL)):
            assert_same(step(e, name), fresh(name), f"step {n} ({name})")
    finally:
        e.close()


def test_create_use_destroy_create_again():
    for n in range(2):
        assert_same(fresh_step(LARGE), fresh(LARGE), f"round {n}")  # (fresh_step returns through close())


def test_the_base_mask_across_a_size_change():
    (cs, mask_s, _, _), (cl, mask_l, pts, cnt) = inputs(SMALL), inputs(LARGE)
    want = dict(fresh(LARGE))
    e = Engine(0)
    try:
        e.clahe_set(*CLAHE)
        resident(e, SMALL)
        e.gft_set_mask(mask_s)
        resident(e, LARGE)
        kept, corners = np.full(60, -7, np.int32), np.full((150, 2), -7.0, np.float32)
        r = e.gft_detect(pts, cnt, min_distance=10, mask_radius=10, kept=kept, corners=corners, check=False)
        assert r["rc"] == -1 and r["num_candidates"] == -1 and np.all(kept == -7) and np.all(corners == -7.0)  # refused, as before
        assert e.gft_set_mask(mask_s, check=False) == -1  # ... and the small mask is not accepted again under the large image
        e.gft_set_mask(mask_l)
        e.klt_track(cl["img1"], NO_POINTS, win_size=cl["win"])  # the image fresh(LARGE) detects on
        d = e.gft_detect(pts, cnt, min_distance=10, mask_radius=10)
        assert d["kept"].tobytes() == want["gft kept"] and d["corners"].tobytes() == want["gft corners"]
        assert (d["num_candidates"], np.float64(d["max_response"]).tobytes()) == want["gft counts"]
    finally:
        e.close()
