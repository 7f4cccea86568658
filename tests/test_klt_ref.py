"""CPU tests of the specification of lfvio_klt_track: tests/klt_ref.py (the float64 numpy restatement of pyramidal Lucas-Kanade,
DESIGN.md 3k), its fixture tests/golden/klt_cases.npz, and lf-vio_amd/csrc/klt_plan.h — plain C++, compiled here alone with g++ behind
a small ctypes shim, as tests/test_window_pack.py does for window_pack.h.

  1  the restatement reproduces its fixture bit for bit, and the fixture is what tests/golden/gen_klt.py writes;
  2  levels: sizes and levels_used of the shapes (a)-(e); pyr_down against a direct double loop on 9 x 7 and 16 x 16; the reflect rule
     against an index-by-index reflect-101 on a 6 x 5 array extended by 13 (more than twice its size: repeated reflection);
  3  on the pure shifts (a), (c), (d) every point has status 1 and lies within 0.05 px of the true flow (the bar: 1.5 x the 0.033 px a
     prototype of the restatement reached on these shapes; the committed restatement reaches 0.043 px);
  4  status: windows in a flat part of the image, a window starting left of -win, textured points, points tracked out of the border
     with border = 1 and border = -1;
  5  klt_plan.h: level sizes, levels_used and offsets equal the restatement's for (a)-(e) and 1280 x 960; every argument limit of
     LfvioKltIn is refused, the limits themselves are accepted;
  6  include/lfvio.h declares lfvio_klt_track / _reset / _level and the built library exports them."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import klt_ref as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {  # case -> the sizes of levels 0 .. levels_used
    "a": [(345, 339), (173, 170), (87, 85), (44, 43)],
    "b": [(345, 339), (173, 170), (87, 85), (44, 43)],
    "c": [(161, 123), (81, 62)],
    "d1": [(177, 185), (89, 93), (45, 47), (23, 24)],
    "d2": [(177, 185), (89, 93), (45, 47), (23, 24)],
    "e": [(97, 75), (49, 38)],
}
BUILT = {}


def built():
    """What gen_klt.py writes, computed once and shared."""
    if not BUILT:
        spec = importlib.util.spec_from_file_location("gen_klt", os.path.join(GOLDEN, "gen_klt.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        BUILT.update(gen.build())
        BUILT["__seeds__"] = gen.SEEDS
    return BUILT


def test_restatement_reproduces_its_fixture():
    b = built()
    with np.load(os.path.join(GOLDEN, "klt_cases.npz")) as z:
        assert sorted(z.files) == sorted(key for key in b if key != "__seeds__")
        for key in z.files:
            assert z[key].dtype == b[key].dtype and z[key].shape == b[key].shape and z[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("case", sorted(k.CASES))
def test_level_sizes(case):
    w, h, win, _, _, _, lu, _ = k.CASES[case]
    p = k.plan(w, h, win, 3)
    assert p["sizes"] == SHAPES[case] and p["levels_used"] == lu == len(SHAPES[case]) - 1
    levels = k.pyramid(np.zeros((h, w), np.uint8), win, 3)
    assert [(l.shape[1], l.shape[0]) for l in levels] == SHAPES[case]
    assert k.plan(w, h, win, 0)["levels_used"] == 0 and k.plan(w, h, win, 5)["levels_used"] >= lu


def loop_reflect(i, n):
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


@pytest.mark.parametrize("w,h", [(9, 7), (16, 16)])
def test_pyr_down_against_a_double_loop(w, h):
    img = np.random.default_rng([w, h]).integers(0, 256, (h, w)).astype(np.uint8)
    kern = (1, 4, 6, 4, 1)
    want = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for y in range(want.shape[0]):
        for x in range(want.shape[1]):
            s = sum(kern[j] * kern[i] * int(img[loop_reflect(2 * y - 2 + j, h), loop_reflect(2 * x - 2 + i, w)]) for j in range(5) for i in range(5))
            want[y, x] = (s + 128) >> 8
    assert np.array_equal(k.pyr_down(img), want)
    assert np.array_equal(k.pyr_down(np.full((h, w), 255, np.uint8)), np.full(want.shape, 255, np.uint8))  # (the weights sum to 256)


def test_reflect_rule():
    a = np.arange(30, dtype=np.uint8).reshape(5, 6)
    e = k.extend(a, 13)
    assert e.shape == (31, 32)
    for y in range(-13, 5 + 13):
        for x in range(-13, 6 + 13):
            assert e[y + 13, x + 13] == a[loop_reflect(y, 5), loop_reflect(x, 6)], (x, y)
    assert k.reflect101(np.array([-1, 0, 5, 6, 7]), 6).tolist() == [1, 0, 5, 4, 3]


def test_gradients_are_scharr_over_32():
    img = np.tile(np.arange(0, 80, 8, dtype=np.uint8), (6, 1))  # a ramp of 8 grey levels per pixel in x
    gx, gy = k.gradients(img)
    assert np.all(gx[:, 1:-1] == 8.0) and np.all(gx[:, 0] == 0.0) and np.all(gx[:, -1] == 0.0) and np.all(gy == 0.0)  # (16 * (2 * 8) / 32: grey levels per pixel; 0 at the edge by reflect-101)
    gx, gy = k.gradients(img.T.copy())
    assert np.all(gy[1:-1, :] == 8.0) and np.all(gx == 0.0)


def test_pure_shifts_reach_the_true_flow():
    b = built()
    worst = 0.0
    for case in k.PURE_SHIFTS:
        for seed in b["__seeds__"]:
            key = f"{case}_{seed}"
            c = k.make_case(case, seed)
            assert np.array_equal(c["pts"], b[key + "_pts"])
            assert np.all(b[key + "_status"] == 1), key
            assert np.all(b[key + "_iterations"] < 30), key
            err = np.hypot(*(b[key + "_next"].astype(np.float64) - c["true"]).T)
            print(f"{key}: worst distance to the true flow {err.max():.4f} px")
            worst = max(worst, err.max())
            assert err.max() <= 0.05, (key, err.max())
    print(f"all pure shifts: {worst:.4f} px")


def test_status():
    b = built()
    on, off = b["status_b1_status"], b["status_bm1_status"]
    assert np.array_equal(on, k.STATUS_WANT)
    assert on[:3].tolist() == [0, 0, 0] and off[:3].tolist() == [0, 0, 0]  # flat windows: minEig below the threshold at level 0
    assert on[3] == 0 and off[3] == 0  # (-50, 10): the window's corner is left of -win at level 0
    assert on[4:6].tolist() == [1, 1] and off[4:6].tolist() == [1, 1]  # textured
    nxt = b["status_b1_next"]
    assert np.array_equal(nxt, b["status_bm1_next"])  # next_pts does not depend on the border test, and is written for status 0 too
    assert np.all(np.rint(nxt[6:, 1]) < 1) and on[6:].tolist() == [0, 0, 0] and off[6:].tolist() == [1, 1, 1]
    assert b["status_b1_counts"].tolist() == [3, 2] and b["status_bm1_counts"].tolist() == [3, 5]
    assert np.all(b["status_b1_iterations"][3, :1] == 0)  # a skipped level runs no iteration


# ---- klt_plan.h behind a ctypes shim
SRC = r'''
#include "klt_plan.h"
extern "C" int kp_plan(int w, int h, int win, int max_level, int *ws, int *hs, long long *off, long long *bytes) {
  const KltPlan p = klt_plan(w, h, win, max_level);
  for (int k = 0; k <= p.levels_used; k++) ws[k] = p.w[k], hs[k] = p.h[k], off[k] = (long long)p.off[k];
  *bytes = (long long)p.bytes;
  return p.levels_used;
}
static unsigned char PIXEL;
static float POINT[2];
extern "C" const char *kp_check(int w, int h, int null_image, int n, int null_pts, int win, int max_level, int max_iter, double eps, double min_eig, int border) {
  LfvioKltIn in;
  in.width = w, in.height = h, in.image = null_image ? nullptr : &PIXEL, in.num_points = n, in.prev_pts = null_pts ? nullptr : POINT;
  in.win_size = win, in.max_level = max_level, in.max_iterations = max_iter, in.epsilon = eps, in.min_eig_threshold = min_eig, in.border = border;
  return klt_check(&in);
}
extern "C" int kp_consts(int *out) {
  const int v[] = {LFVIO_KLT_MAX_POINTS, LFVIO_KLT_MAX_LEVEL, KLT_LEVELS, (int)KLT_ALIGN, (int)sizeof(LfvioKltIn), (int)sizeof(LfvioKltOut)};
  for (unsigned k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
  return (int)(sizeof v / sizeof v[0]);
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="klt_plan_")
    src, so = os.path.join(d, "kp.cpp"), os.path.join(d, "libkp.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.kp_plan.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4
    so.kp_check.restype = C.c_char_p
    so.kp_check.argtypes = [C.c_int] * 8 + [C.c_double] * 2 + [C.c_int]
    return so


@pytest.mark.parametrize("w,h,win", [k.CASES[c][:3] for c in sorted(k.CASES)] + [(1280, 960, 41), (1280, 960, 21), (16, 16, 41), (8192, 8192, 5)])
def test_plan_header_against_the_restatement(lib, w, h, win):
    for max_level in range(k.MAX_LEVEL + 1):
        ws, hs, off, nbytes = (C.c_int * 6)(), (C.c_int * 6)(), (C.c_longlong * 6)(), C.c_longlong(0)
        lu = lib.kp_plan(w, h, win, max_level, ws, hs, off, C.byref(nbytes))
        p = k.plan(w, h, win, max_level)
        assert lu == p["levels_used"] and list(zip(ws[:lu + 1], hs[:lu + 1])) == p["sizes"]
        assert list(off[:lu + 1]) == p["offsets"] and nbytes.value == p["bytes"]
    if (w, h, win) == (1280, 960, 41):
        assert k.plan(w, h, win, 3)["sizes"] == [(1280, 960), (640, 480), (320, 240), (160, 120)] and k.plan(w, h, win, 5)["levels_used"] == 4


def test_plan_header_constants_and_structs(lib):
    from lfvio import abi

    out = (C.c_int * 8)()
    assert lib.kp_consts(out) == 6
    assert out[:6] == [abi.KLT_MAX_POINTS, abi.KLT_MAX_LEVEL, abi.KLT_MAX_LEVEL + 1, k.ALIGN, C.sizeof(abi.KltInC), C.sizeof(abi.KltOutC)]
    assert (k.MAX_POINTS, k.MAX_LEVEL) == (abi.KLT_MAX_POINTS, abi.KLT_MAX_LEVEL)


GOOD = dict(w=345, h=339, null_image=0, n=65, null_pts=0, win=41, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4, border=1)
ORDER = ("w", "h", "null_image", "n", "null_pts", "win", "max_level", "max_iter", "eps", "min_eig", "border")
REFUSED = [dict(w=15), dict(w=8193), dict(h=15), dict(h=8193), dict(null_image=1), dict(n=-1), dict(n=4097), dict(null_pts=1), dict(win=3), dict(win=4),
           dict(win=40), dict(win=43), dict(max_level=-1), dict(max_level=6), dict(max_iter=0), dict(max_iter=101), dict(eps=0.0), dict(eps=-0.01),
           dict(eps=float("nan")), dict(min_eig=-1e-9), dict(min_eig=float("nan"))]
ACCEPTED = [dict(), dict(w=16, h=16), dict(w=8192, h=8192), dict(n=0), dict(n=0, null_pts=1), dict(n=4096), dict(win=5), dict(max_level=0), dict(max_level=5),
            dict(max_iter=1), dict(max_iter=100), dict(eps=1e-300), dict(min_eig=0.0), dict(border=-1), dict(border=0), dict(border=1000)]


def test_argument_limits(lib):
    check = lambda over: lib.kp_check(*[dict(GOOD, **over)[f] for f in ORDER])
    for over in ACCEPTED:
        assert check(over) is None, over
    for over in REFUSED:
        why = check(over)
        assert why is not None and why.startswith(b"lfvio_klt_track: "), over


def test_header_declares_and_library_exports():
    import __graft_entry__ as ge

    ge.build()
    from lfvio import abi

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfvio.h")).read(), flags=re.S)
    lib = C.CDLL(abi.HIP_LIB_PATH)
    for name in ("lfvio_klt_track", "lfvio_klt_reset", "lfvio_klt_level"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+LFVIO_KLT_MAX_POINTS\s+4096\b", src) and re.search(r"#define\s+LFVIO_KLT_MAX_LEVEL\s+5\b", src)
