"""CPU tests of the image encodings: lf-vio_amd/csrc/image_format.h (compiled alone with g++, behind a ctypes shim) held to its
restatement tests/image_ref.py, and the recordings' route — rosmsg, trace, tools/bag_to_lfvt.py, the host loader.

  1  the grey functions: all 65 536 16-bit values in both byte orders, all 2^24 bgr8 triples, 2^20 seeded pixels each of rgb8, bgra8,
     rgba8 (the alpha byte never shows); the integer 16-bit line equals cv_bridge's float product in float32 and in double, with no
     float32 product on a tie; where the rounded floating colour formula differs from the fixed-point line, the header sides with
     the fixed-point line
  2  the whole-image host converter at odd sizes and steps, the padding seeded noise
  3  imgfmt_check: every refusal and every acceptance, against image_ref.check
  4  ser_image_raw -> de_image_any for the seven names and big-endian mono16; a bag with a bgr8 and a mono16 topic through
     bag_to_lfvt.convert and read_trace; the CPU build's loader on code-2 records, a short step, mixed codes and codes 1 and 8"""
import ctypes as C
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import image_ref as ir
from lfvio import abi, rosmsg, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SRC = r'''
#include "image_format.h"
extern "C" {
int if_bpp(int code) { return imgfmt_bpp(code); }
const char *if_check(int code, int step, int width, int height) { return imgfmt_check(LfvioImageFormat{code, step}, width, height); }
// n pixels of bpp bytes each, back to back
void if_pixels(int code, long n, const unsigned char *px, unsigned char *out) {
  const int bpp = imgfmt_bpp(code);
  for (long i = 0; i < n; i++, px += bpp) out[i] = (unsigned char)imgfmt_gray(code, px[0], bpp > 1 ? px[1] : 0u, bpp > 2 ? px[2] : 0u);
}
void if_image(int code, int width, int height, long step, const unsigned char *src, unsigned char *dst) { imgfmt_to_gray(code, width, height, (size_t)step, src, dst); }
// {code, step, bytes, convert} of imgfmt_plan; code < 0: no format
void if_plan(int code, int step, int width, int height, long *out) {
  const LfvioImageFormat f = {code, step};
  const ImgfmtPlan p = imgfmt_plan(code < 0 ? nullptr : &f, width, height);
  out[0] = p.code, out[1] = (long)p.step, out[2] = (long)p.bytes, out[3] = p.convert;
}
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="image_format_")
    src, so = os.path.join(d, "if.cpp"), os.path.join(d, "libif.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    up = C.POINTER(C.c_ubyte)
    so.if_check.restype = C.c_char_p
    so.if_check.argtypes = [C.c_int] * 4
    so.if_pixels.argtypes = [C.c_int, C.c_long, up, up]
    so.if_image.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, up, up]
    so.if_plan.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_long)]
    return so


def _u(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def header_pixels(lib, code, px):
    px = np.ascontiguousarray(px, dtype=np.uint8).reshape(-1, ir.BPP[code])
    out = np.full(len(px), 0xA5, np.uint8)
    lib.if_pixels(code, len(px), _u(px), _u(out))
    return out


# ---- 1
def test_codes_and_bytes_per_pixel(lib):
    for code in range(-2, 12):
        assert lib.if_bpp(code) == ir.BPP.get(code, 0), code
    assert abi.IMG_BPP == ir.BPP and rosmsg.IMAGE_BPP == ir.BPP
    assert (abi.IMG_MONO8, abi.IMG_BGR8, abi.IMG_RGB8, abi.IMG_BGRA8, abi.IMG_RGBA8, abi.IMG_MONO16, abi.IMG_MONO16_BE) == ir.CODES


def test_sixteen_bits_exhaustive(lib):
    v = np.arange(65536, dtype=np.int64)
    want = ir.gray_16(v)
    lo, hi = (v & 255).astype(np.uint8), (v >> 8).astype(np.uint8)
    assert np.array_equal(header_pixels(lib, ir.MONO16, np.stack([lo, hi], 1)), want)
    assert np.array_equal(header_pixels(lib, ir.MONO16_BE, np.stack([hi, lo], 1)), want)
    assert want[0] == 0 and want[128] == 0 and want[129] == 1 and want[65535] == 255 and want[65407] == 255 and want[65406] == 254
    # the four forms of the issue: float32 product, the same in double, the integer form; no float32 product is a tie
    assert np.array_equal(ir.gray_16_float(v, np.float32), want) and np.array_equal(ir.gray_16_float(v, np.float64), want)
    prod = v.astype(np.float32) * np.float32(255.0 / 65535.0)
    assert not (prod - np.floor(prod) == np.float32(0.5)).any()


def test_bgr8_exhaustive(lib):
    c = np.arange(256, dtype=np.uint8)
    for b in range(0, 256, 32):  # 2^24 triples in eight slabs of 2^21
        bb, gg, rr = np.meshgrid(c[b:b + 32], c, c, indexing="ij")
        px = np.stack([bb.ravel(), gg.ravel(), rr.ravel()], 1)
        assert np.array_equal(header_pixels(lib, ir.BGR8, px), ir.gray_bgr(px[:, 0], px[:, 1], px[:, 2])), b
    assert ir.gray_bgr(255, 255, 255) == 255 and ir.gray_bgr(0, 0, 0) == 0 and 1868 + 9617 + 4899 == 1 << 14


@pytest.mark.parametrize("code", [ir.RGB8, ir.BGRA8, ir.RGBA8])
def test_seeded_pixels_and_alpha(lib, code):
    rng = np.random.default_rng(code)
    bpp = ir.BPP[code]
    px = rng.integers(0, 256, (1 << 20, bpp), dtype=np.uint8)
    b, r = (px[:, 0], px[:, 2]) if code == ir.BGRA8 else (px[:, 2], px[:, 0])
    want = ir.gray_bgr(b, px[:, 1], r)
    got = header_pixels(lib, code, px)
    assert np.array_equal(got, want) and np.array_equal(ir.to_gray(px.reshape(1024, -1), 1024, code).ravel(), want)
    if bpp == 4:
        other = px.copy()
        other[:, 3] = rng.integers(0, 256, len(px), dtype=np.uint8)
        assert (other[:, 3] != px[:, 3]).mean() > 0.9 and np.array_equal(header_pixels(lib, code, other), got)


def test_header_sides_with_the_fixed_point_line(lib):
    px = np.random.default_rng(7).integers(0, 256, (10 ** 6, 3), dtype=np.uint8)
    fixed, floating = ir.gray_bgr(px[:, 0], px[:, 1], px[:, 2]), ir.gray_bgr_float(px[:, 0], px[:, 1], px[:, 2])
    differ = fixed != floating
    assert 0.0005 < differ.mean() < 0.005  # (the issue measured about 0.18 %)
    assert np.abs(fixed.astype(int) - floating.astype(int)).max() == 1
    assert np.array_equal(header_pixels(lib, ir.BGR8, px[differ]), fixed[differ])
    assert np.array_equal(header_pixels(lib, ir.RGB8, px[differ][:, ::-1]), fixed[differ])


# ---- 2
SHAPES = [(16, 16, 0), (17, 19, 1), (17, 19, 3), (64, 48, 5), (80, 60, None)]  # (w, h, step - w * bpp; None: step 512)


def step_of(w, pad, code):
    return 512 if pad is None else w * ir.BPP[code] + pad


@pytest.mark.parametrize("code", ir.CODES)
@pytest.mark.parametrize("w,h,pad", SHAPES)
def test_host_converter(lib, code, w, h, pad):
    step = step_of(w, pad, code)
    assert step >= w * ir.BPP[code]
    rows = np.random.default_rng(100 * code + w + h + step).integers(0, 256, (h, step), dtype=np.uint8)
    want = ir.to_gray(rows, w, code)
    out = np.full((h + 1, w), 0x5A, np.uint8)  # one row more: nothing is written behind the image
    lib.if_image(code, w, h, step, _u(rows), _u(out))
    assert np.array_equal(out[:h], want) and (out[h] == 0x5A).all()
    noisy = rows.copy()
    noisy[:, w * ir.BPP[code]:] ^= 0xFF  # other padding, the same image
    lib.if_image(code, w, h, step, _u(noisy), _u(out))
    assert np.array_equal(out[:h], want)
    assert np.array_equal(ir.to_gray(ir.from_gray(want, code, step, seed=3), w, code).shape, (h, w))


# ---- 3
def test_check_function(lib):
    def refused(code, step, w=64, h=48):
        why = lib.if_check(code, step, w, h)
        assert (why is None) == (ir.check(code, step, w) is None), (code, step, w, why)
        return why is not None

    for code in (-1, 1, 8, 9, 255):
        assert refused(code, 0) and refused(code, 640)
    for code in ir.CODES:
        bpp = ir.BPP[code]
        assert refused(code, -1) and refused(code, 65537) and refused(code, 64 * bpp - 1) and refused(code, 1)
        assert not refused(code, 0) and not refused(code, 64 * bpp) and not refused(code, 64 * bpp + 5) and not refused(code, 65536)
        for w, h in ((15, 48), (8193, 48), (64, 15), (64, 8193)):
            assert lib.if_check(code, 0, w, h) is not None
        assert lib.if_check(code, 0, 16, 16) is None and lib.if_check(code, 0, 8192 if bpp * 8192 <= 65536 else 64, 8192) is None


def test_plan(lib):
    def plan(code, step, w=64, h=48):
        o = (C.c_long * 4)()
        lib.if_plan(code, step, w, h, o)
        return tuple(o)

    none = plan(-1, 0)
    assert none == (0, 64, 64 * 48, 0) and plan(ir.MONO8, 0) == none and plan(ir.MONO8, 64) == none  # mono8, contiguous: no format
    assert plan(ir.MONO8, 70) == (0, 70, 70 * 48, 1)
    for code in ir.CODES[1:]:
        bpp = ir.BPP[code]
        assert plan(code, 0) == (code, 64 * bpp, 64 * bpp * 48, 1) and plan(code, 64 * bpp + 5) == (code, 64 * bpp + 5, (64 * bpp + 5) * 48, 1)


# ---- 4
NAMES = [(b"mono8", 0, 0), (b"8UC1", 0, 0), (b"bgr8", 0, 2), (b"rgb8", 0, 3), (b"bgra8", 0, 4), (b"rgba8", 0, 5), (b"mono16", 0, 6), (b"mono16", 1, 7)]


@pytest.mark.parametrize("name,big,code", NAMES)
def test_message_round_trip(name, big, code):
    w, h = 24, 17
    step = w * ir.BPP[code] + 3
    rows = np.random.default_rng(code + 10 * big).integers(0, 256, (h, step), dtype=np.uint8)
    stamp, got, gw, gstep, gcode = rosmsg.de_image_any(rosmsg.ser_image_raw(4, 31.5, rows, w, name, is_bigendian=big))
    assert (stamp, gw, gstep, gcode) == (31.5, w, step, code) and np.array_equal(got, rows)
    if code == 0:  # the existing reader sees the same message
        st, img, s2, enc = rosmsg.de_image(rosmsg.ser_image_raw(4, 31.5, rows, w, name))
        assert (st, s2, enc) == (31.5, step, name.decode()) and np.array_equal(img, rows[:, :w])
    else:
        with pytest.raises(ValueError):
            rosmsg.de_image(rosmsg.ser_image_raw(4, 31.5, rows, w, name, is_bigendian=big))
    with pytest.raises(ValueError):  # a row shorter than its pixels
        rosmsg.de_image_any(rosmsg.ser_image_raw(4, 31.5, rows[:, :w * ir.BPP[code] - 1], w, name, is_bigendian=big))


def test_messages_that_are_refused():
    rows = np.zeros((16, 64), np.uint8)
    for name in (b"bayer_rggb8", b"8UC3", b"16UC1", b"32FC1", b"rgb16", b""):
        with pytest.raises(ValueError):
            rosmsg.de_image_any(rosmsg.ser_image_raw(0, 1.0, rows, 16, name))


def test_bag_with_colour_and_sixteen_bit_topics(tmp_path):
    import bag_to_lfvt

    bag = str(tmp_path / "cam.bag")
    w, h = 48, 32
    rng = np.random.default_rng(5)
    colour = [rng.integers(0, 256, (h, w * 3 + 4), dtype=np.uint8) for _ in range(3)]
    deep = [rng.integers(0, 256, (h, w * 2), dtype=np.uint8) for _ in range(3)]
    bw = rosmsg.BagWriter(bag, chunk_messages=4)
    for k in range(3):
        t = 50.0 + 0.1 * k
        bw.write("/imu0", "sensor_msgs/Imu", t - 0.02, rosmsg.ser_imu(k, t - 0.02, [0.0, 0.0, 9.8], [0.0, 0.0, 0.0]))
        bw.write("/colour/image_raw", "sensor_msgs/Image", t, rosmsg.ser_image_raw(k, t, colour[k], w, b"bgr8"))
        bw.write("/deep/image_raw", "sensor_msgs/Image", t, rosmsg.ser_image_raw(k, t, deep[k], w, b"mono16"))
    bw.close()
    for topic, raws, code in (("/colour/image_raw", colour, ir.BGR8), ("/deep/image_raw", deep, ir.MONO16)):
        out = str(tmp_path / f"cam{code}.lfvt")
        n = bag_to_lfvt.convert(bag, out, image_topic=topic)
        assert n["raw_images"] == 3 and n["imu"] == 3 and n["other"] == 3
        t = trace.read_trace(out)
        assert t["order"] == [1, 10] * 3 and t["raw_encodings"] == [code] * 3 and t["raw_steps"] == [raws[0].shape[1]] * 3
        for k, (stamp, img) in enumerate(t["raw_images"]):
            assert abs(stamp - (50.0 + 0.1 * k)) < 1e-9
            want = ir.typed(raws[k], w, code)
            assert img.dtype == want.dtype and img.shape == want.shape and np.array_equal(img, want)
        assert t["raw_images"][0][1].shape == ((h, w, 3) if code == ir.BGR8 else (h, w))
        # the rows went through unchanged, padding included
        body = open(out, "rb").read()
        assert body.count(raws[1].tobytes()) == 1


def test_writer_reader_every_encoding(tmp_path):
    p = str(tmp_path / "enc.lfvt")
    w, h = 20, 16
    for code in ir.CODES:
        rows = np.random.default_rng(code).integers(0, 256, (h, w * ir.BPP[code] + 2), dtype=np.uint8)
        tw = trace.TraceWriter(p)
        if code == 0:
            tw.image(1.0, rows[:, :w], step=rows.shape[1])
        else:
            tw.image(1.0, rows, encoding=code, width=w)
        tw.close()
        t = trace.read_trace(p)
        assert t["raw_encodings"] == [code] and t["raw_steps"] == [rows.shape[1]]
        assert np.array_equal(t["raw_images"][0][1], ir.typed(rows, w, code))
    v = ir.typed(np.array([[0x34, 0x12] * 16] * 16, np.uint8), 16, ir.MONO16)
    assert v.dtype == np.uint16 and v[0, 0] == 0x1234 and ir.typed(np.array([[0x12, 0x34] * 16] * 16, np.uint8), 16, ir.MONO16_BE)[0, 0] == 0x1234


def image_record(t=1.0, w=32, h=16, step=None, enc=2):
    step = w * ir.BPP.get(enc, 1) if step is None else step
    body = struct.pack("<dIIII", t, w, h, step, enc) + bytes(h * step)
    return struct.pack("<II", 10, len(body)) + body


def test_cpu_loader_takes_the_codes(oracle, tmp_path):
    from lfvio.host import HostEstimator

    head = b"LFVT" + struct.pack("<I", 1)
    cpu = HostEstimator(oracle.build_host_oracle())
    try:
        def rc(body):
            p = str(tmp_path / "t.lfvt")
            open(p, "wb").write(head + body)
            return cpu.replay(p)[0]

        assert rc(image_record() + image_record(t=1.1, step=32 * 3 + 7)) == 0
        for code in ir.CODES:
            assert rc(image_record(enc=code) + image_record(t=1.1, enc=code, step=32 * ir.BPP[code] + 1)) == 0, code
            assert rc(image_record(enc=code, step=32 * ir.BPP[code] - 1)) == -3, code
        assert rc(image_record(step=3 * 32 - 1)) == -3
        assert rc(image_record(enc=0) + image_record(t=1.1, enc=2)) == -3 and rc(image_record(enc=2) + image_record(t=1.1, enc=0, step=96)) == -3
        assert rc(image_record(enc=1)) == -3 and rc(image_record(enc=8)) == -3 and rc(image_record(enc=0xFFFFFFFF, step=32)) == -3
        assert rc(image_record(enc=0, step=65537)) == -3 and rc(image_record(enc=0, step=65536)) == 0
    finally:
        cpu.close()
