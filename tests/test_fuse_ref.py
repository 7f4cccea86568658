"""CPU tests of lfvio_cloud_fuse's specification (tests/fuse_ref.py) against mpmath at 50 digits on the REFERENCE's definition
(pointcloud_image_fusion_node.cpp:92-115): P = R p + T, normalised; lon = atan2(x, y), lat = asin(z); fx = cols (0.5 + lon / (2 pi)),
fy = rows (0.5 - lat / pi); idx_x = (int)fx, idx_y = (int)fy.  CAMERA's projection is what tests/test_project_ref.py already holds.

  1  the fractional pixel (fx, fy) of 20 000 seeded float32 points over the whole sphere at 0.3 .. 120 m through three poses (the
     identity; the node's R with theta = pi / 2 and T = (0, 0, -0.12); a random rotation with an offset), at 960 x 480 and 8192 x 4096,
     in units of eps max(width, height):                                  measured 32.134  bar 64.268
     (the bar is TWICE the measured maximum, DESIGN.md 3x.  The unit is large beside the projections' because a point near a pole has
     its longitude from a short (X, Y): the rounding of R p + T, about eps |P|, is divided by nxy.)
  2  col, row equal the 50-digit indices for every point whose 50-digit fx and fy both lie further than the bar from an integer; NO
     point of these seeds lies that close (at 64.268 eps 8192 = 1.2e-10 px the expected count among 120 000 is 6e-5), which the test
     checks, so every index is compared — far inside the 1 in 1 000 the specification allows to be left out
  3  hand-made points with exact expectations: both sides of the seam (X = +-tiny, Y < 0), X = 0 with Y < 0 exactly (column 0), the
     four axis directions, both poles (dropped), |Z / nxy| >= 2^66 (row height - 1, or row 0 above), the zero point and NaN / inf (the gate)
  4  consistency with the map: for 1 000 rays of project_ref.equirect_rays at pixel centres (i + 0.5, j + 0.5) the index is (i, j)
  5  the range gate's two ends hit exactly, and the range image: the minimum per pixel whatever the order
  6  tests/golden/fuse_cases.npz regenerates byte for byte"""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

import fuse_ref as fr
import project_ref as pr

EPS = 2.0 ** -52
BAR_FRAC = 64.268  # eps max(width, height); twice the measured 32.134
SIZES = ((960, 480), (8192, 4096))


def frac50(R, T, P):
    """The reference's (fx / cols, fy / rows) of every point at 50 digits: lists of mpf."""
    mp.mp.dps = 50
    Rm = [[mp.mpf(float(v)) for v in row] for row in np.asarray(R).reshape(3, 3)]
    Tm = [mp.mpf(float(v)) for v in T]
    two_pi = 2 * mp.pi
    out = []
    for p in P:
        q = [mp.mpf(float(v)) for v in p]
        X, Y, Z = (Rm[k][0] * q[0] + Rm[k][1] * q[1] + Rm[k][2] * q[2] + Tm[k] for k in range(3))
        n = mp.sqrt(X * X + Y * Y + Z * Z)
        out.append((mp.mpf(0.5) + mp.atan2(X / n, Y / n) / two_pi, mp.mpf(0.5) - mp.asin(Z / n) / mp.pi))
    return out


@pytest.fixture(scope="module")
def sphere():
    """Per pose: the cloud, the 50-digit unit fractions and, per size, the numpy text's (fx, fy, index).  Computed once."""
    P = fr.sphere_cloud(20000)
    out = {}
    for name, R, T in fr.poses():
        ref = frac50(R, T, P)
        X, Y, Z = fr.transform(R, T, P[:, 0], P[:, 1], P[:, 2])
        got = {}
        for W, H in SIZES:
            fx, fy = fr.equirect_frac(W, H, X, Y, Z)
            got[W, H] = fx, fy, fr.points(fr.view(width=W, height=H, R=R, T=T), P[:, 0], P[:, 1], P[:, 2])[0]
        out[name] = P, ref, got
    return out


# ---- 1
def test_fractional_pixel_against_50_digits(sphere):
    worst = 0.0
    for name, (P, ref, got) in sphere.items():
        for (W, H), (fx, fy, _) in got.items():
            unit = mp.mpf(EPS * max(W, H))
            w = max(max(abs(mp.mpf(float(a)) - W * u), abs(mp.mpf(float(b)) - H * v)) for a, b, (u, v) in zip(fx, fy, ref))
            print(f"fuse equirect {name} {W} x {H}: {float(w / unit):.3f} eps max(width, height) = {float(w):.3e} px")
            worst = max(worst, float(w / unit))
    print(f"fuse equirect: {worst:.3f} eps max(width, height) (bar {BAR_FRAC})")
    assert worst <= BAR_FRAC


# ---- 2
def test_indices_against_50_digits(sphere):
    for name, (P, ref, got) in sphere.items():
        for (W, H), (_, _, index) in got.items():
            bar = mp.mpf(BAR_FRAC * EPS * max(W, H))
            near, want = 0, np.zeros(len(P), np.int64)
            for k, (u, v) in enumerate(ref):
                fx, fy = W * u, H * v
                near += abs(fx - mp.nint(fx)) <= bar or abs(fy - mp.nint(fy)) <= bar
                want[k] = int(mp.floor(fy)) * W + int(mp.floor(fx))  # both positive: (int) truncates as floor
            # these seeds put no 50-digit coordinate within the bar of an integer: nothing is left out of the comparison
            assert near == 0, (name, W, H, near)
            assert np.array_equal(index, want), (name, W, H)


# ---- 3
def idx(points, W=960, H=480, **kw):
    P = np.asarray(points, np.float32).reshape(-1, 3)
    return fr.points(fr.view(width=W, height=H, **kw), P[:, 0], P[:, 1], P[:, 2])


def test_hand_made_points():
    W, H = 960, 480
    mid = (H // 2) * W  # Z == 0: lat = 0, fy = height / 2 exactly
    # the seam: lon = +-pi behind the camera.  X = +tiny gives fx = width (wrapped to column 0), X = -tiny gives fx = 0
    i, _, why = idx([[1e-30, -1.0, 0.0], [-1e-30, -1.0, 0.0], [0.0, -1.0, 0.0], [-0.0, -1.0, 0.0]])
    assert i.tolist() == [mid, mid, mid, mid] and not why.any()
    # a little further from it: the last column on the +X side, the first on the -X side
    i, _, _ = idx([[1e-3, -1.0, 0.0], [-1e-3, -1.0, 0.0]])
    assert i.tolist() == [mid + W - 1, mid]
    # the axes: +Y the centre column, +X three quarters, -X one quarter, -Y column 0
    i, _, _ = idx([[0.0, 2.0, 0.0], [2.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    assert i.tolist() == [mid + W // 2, mid + 3 * W // 4, mid + W // 4, mid]
    # the poles are dropped by the projection, the zero point and what is not finite by the gate
    i, r, why = idx([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0], [0.0, 0.0, 0.0], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf]])
    assert i.tolist() == [-1] * 6 and why.tolist() == [fr.PROJECTION, fr.PROJECTION] + [fr.GATE] * 4 and r[0] == 3.0 and r[2] == 0.0
    # the largest float32 values stay finite in double: the point is kept
    assert idx([[3e38, 3e38, 1.0]])[2].tolist() == [fr.KEPT]
    # |Z / nxy| >= 2^66: lat = -+pi / 2 as a double, fy = height below (row height - 1) and 0 above; nxy = 1e-25 is off the pole
    i, _, why = idx([[0.0, 1e-25, -1.0], [0.0, 1e-25, 1.0], [1e-25, 0.0, -1.0]])
    assert 1.0 / 1e-25 >= 2.0 ** 66 and i.tolist() == [(H - 1) * W + W // 2, W // 2, (H - 1) * W + 3 * W // 4] and not why.any()
    # the same on a size that is no power of two, through the node's pose: R takes (x, y, z) to (-y, x, z) up to cos(pi / 2) = 6e-17
    i, _, _ = idx([[2.0, 0.0, 0.12], [0.0, -2.0, 0.12]], W=33, H=17, R=fr.node_R(), T=fr.NODE_T)
    assert i.tolist() == [8 * 33 + 16, 8 * 33 + 24]


# ---- 4
def test_pixel_centres_of_the_map_come_back():
    W, H = 128, 64
    rays = pr.equirect_rays(2 * W, 2 * H)  # entry (2 j + 1, 2 i + 1) is the ray of (i + 0.5, j + 0.5) at W x H
    rng = np.random.default_rng(405)
    i, j = rng.integers(0, W, 1000), rng.integers(0, H, 1000)
    P = (rays[2 * j + 1, 2 * i + 1] * rng.uniform(0.5, 50.0, (1000, 1))).astype(np.float32)
    index, _, why = idx(P, W=W, H=H)
    assert not why.any() and np.array_equal(index, j * W + i)


# ---- 5
def test_gate_and_range_image():
    P = np.array([[0.0, 3.0, 4.0], [0.0, 6.0, 8.0], [0.0, 1.5, 2.0]], np.float32)  # r = 5, 10, 2.5 exactly, one direction
    for lo, hi, want in ((5.0, 10.0, [0, 0, 1]), (np.nextafter(5.0, 6.0), 10.0, [1, 0, 1]), (5.0, np.nextafter(10.0, 0.0), [0, 1, 1]), (0.0, np.inf, [0, 0, 0]),
                         (2.5, 2.5, [1, 1, 0])):
        i, r, why = idx(P, W=33, H=17, min_range=lo, max_range=hi)
        assert why.tolist() == want and r.tolist() == [5.0, 10.0, 2.5] and ((i >= 0) == (why == 0)).all()
    i, r, _ = idx(P, W=33, H=17)
    assert i[0] == i[1] == i[2]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        img = fr.range_image(i[order], r[order], 33, 17)
        assert img.reshape(-1)[i[0]] == 2.5 and np.isinf(img).sum() == 33 * 17 - 1


# ---- 6
def test_fixture_regenerates(golden_dir):
    sys.path.insert(0, golden_dir)
    import gen_fuse

    z = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    fresh = gen_fuse.build()
    assert sorted(z.files) == sorted(fresh)
    for k in z.files:
        a, b = z[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert 200 <= len(z["P"]) <= 999 and z["identity/range"].shape == (17, 33)
    assert os.path.getsize(os.path.join(golden_dir, "fuse_cases.npz")) <= os.path.getsize(os.path.join(golden_dir, "remap_cases.npz"))
