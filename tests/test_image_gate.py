"""CPU tests of the node's gate (lf-vio_amd/host/image_gate.h, compiled alone with g++ behind a small extern "C" shim) against
tests/node_ref.Gate: every decision and every state variable, stamp by stamp.

  1  10, 15, 20 and 30 Hz streams at FREQ 10, a few hundred stamps each, exact and jittered
  2  a gap of exactly 1.0 s and one just above it, a stamp that goes backwards, a repeated stamp, two restarts in a row
  3  properties of the restatement: the image after a restart is dropped, init_pub survives a restart, the first publication is
     skipped once, and the published rate of the 30 Hz stream lies within the band the gate itself enforces"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import node_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "image_gate.h"
using lfvio::ImageGate;
extern "C" void *gate_new(int freq) {
  ImageGate *g = new ImageGate();
  g->freq = freq;
  return g;
}
extern "C" void gate_delete(void *g) { delete (ImageGate *)g; }
// one stamp through onStamp and, where it reached the tracker, afterFrame: out = {stamp decision, frame decision or -1}
extern "C" void gate_step(void *h, double t, int *out, double *state) {
  ImageGate *g = (ImageGate *)h;
  out[0] = g->onStamp(t);
  out[1] = out[0] == ImageGate::TRACK ? (int)g->afterFrame() : -1;
  state[0] = g->first_image_flag, state[1] = g->first_image_time, state[2] = g->last_image_time, state[3] = g->pub_count;
  state[4] = g->init_pub, state[5] = g->publish;
}
'''


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="image_gate_")
    src, so = os.path.join(d, "gate.cpp"), os.path.join(d, "libgate.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "lf-vio_amd", "host"), src, "-o", so])
    so = C.CDLL(so)
    so.gate_new.restype = C.c_void_p
    so.gate_new.argtypes = [C.c_int]
    so.gate_delete.argtypes = [C.c_void_p]
    so.gate_step.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    return so


def restated(stamps, freq=10):
    """-> [(stamp decision, frame decision or -1, state)] of node_ref.Gate."""
    g, out = nr.Gate(freq), []
    for t in stamps:
        a = g.on_stamp(t)
        b = g.after_frame() if a == nr.TRACKED else -1
        out.append((a, b, g.state()))
    return out


def hold(lib, stamps, freq=10):
    """The header against the restatement on one sequence; returns the restatement's list."""
    want = restated(stamps, freq)
    h = lib.gate_new(freq)
    try:
        o, s = (C.c_int * 2)(), (C.c_double * 6)()
        for k, t in enumerate(stamps):
            lib.gate_step(h, float(t), o, s)
            a, b, st = want[k]
            assert (o[0], o[1]) == (a, b), (k, t, list(o), a, b)
            got = (bool(s[0]), s[1], s[2], int(s[3]), bool(s[4]), bool(s[5]))
            assert np.array(got, np.float64).tobytes() == np.array([float(v) for v in st]).tobytes(), (k, t, got, st)
    finally:
        lib.gate_delete(h)
    return want


def stream(hz, n, start=1403636579.76, jitter=0.0, seed=0):
    t = start + np.arange(n) / float(hz)
    if jitter:
        t = t + np.random.default_rng(seed).uniform(-jitter, jitter, n)
    return t.tolist()


@pytest.mark.parametrize("hz", [10, 15, 20, 30])
def test_streams(lib, hz):
    for kw in (dict(), dict(jitter=0.2 / hz, seed=hz), dict(start=0.0)):
        w = hold(lib, stream(hz, 400, **kw))
        assert w[0][0] == nr.DROP and all(a == nr.TRACKED for a, _, _ in w[1:])
        pub = [b for _, b, _ in w if b in (nr.FIRST_PUBLICATION, nr.PUBLISHED)]
        assert pub[0] == nr.FIRST_PUBLICATION and pub.count(nr.FIRST_PUBLICATION) == 1 and len(pub) > 100
        if hz > 10 and not kw:
            assert any(b == nr.TRACKED for _, b, _ in w)  # some frames are tracked only


def test_gaps_backward_and_repeated_stamps(lib):
    base = 100.0
    ten = [base + 0.1 * k for k in range(6)]
    # a gap of exactly 1.0 s is no discontinuity (the test is >), one just above it is
    last = ten[-1]
    w = hold(lib, ten + [last + 1.0, last + 1.1])
    assert [a for a, _, _ in w[-2:]] == [nr.TRACKED, nr.TRACKED]
    w = hold(lib, ten + [np.nextafter(last + 1.0, np.inf) + 1e-9, last + 1.2, last + 1.3])
    assert [a for a, _, _ in w[-3:]] == [nr.RESTART, nr.DROP, nr.TRACKED]
    # a stamp that goes backwards
    w = hold(lib, ten + [last - 0.05, last + 0.1, last + 0.2])
    assert [a for a, _, _ in w[-3:]] == [nr.RESTART, nr.DROP, nr.TRACKED]
    # a repeated stamp: tracked, never published (the rate is inf, or NaN behind a reset of the frequency control)
    w = hold(lib, ten + [last, last + 0.1])
    assert w[-2][:2] == (nr.TRACKED, nr.TRACKED) and w[-1][0] == nr.TRACKED
    w = hold(lib, [base, base, base, base + 0.1])  # right behind the dropped image: 1 / 0
    assert [x[:2] for x in w[:3]] == [(nr.DROP, -1), (nr.TRACKED, nr.TRACKED), (nr.TRACKED, nr.TRACKED)]
    # two restarts in a row: the stamp behind a restart is dropped whatever it is, the next one can restart again
    w = hold(lib, ten + [last + 5.0, last + 5.1, last + 10.0, last + 3.0, last + 3.1, last + 3.2])
    assert [a for a, _, _ in w[-6:]] == [nr.RESTART, nr.DROP, nr.RESTART, nr.DROP, nr.TRACKED, nr.TRACKED]
    # stamps near zero and negative
    hold(lib, [0.0, 0.1, 0.2, -0.1, 0.0, 0.1])
    hold(lib, [-5.0 + 0.1 * k for k in range(80)])


def test_properties_of_the_restatement():
    # the image after a restart is dropped; init_pub survives a restart: the first publication is skipped ONCE
    st = stream(10, 30, start=50.0) + stream(10, 30, start=60.0)
    w = restated(st)
    k = [i for i, (a, _, _) in enumerate(w) if a == nr.RESTART]
    assert k == [30] and w[31][0] == nr.DROP
    assert w[29][2][4] is True and w[30][2][4] is True and w[31][2][4] is True
    frames = [b for _, b, _ in w if b != -1]
    assert frames.count(nr.FIRST_PUBLICATION) == 1 and frames[0] == nr.FIRST_PUBLICATION
    assert w[32][1] == nr.PUBLISHED  # the first image tracked behind the restart goes out
    # pub_count is 1 again behind a restart, first_image_time the dropped stamp
    assert w[30][2][3] == 1 and w[31][2][1] == st[31]
    # a 10 Hz stream at FREQ 10: every image behind the dropped one publishes
    assert all(b in (nr.FIRST_PUBLICATION, nr.PUBLISHED) for _, b, _ in restated(stream(10, 200, start=7.0))[1:])


def test_published_rate_of_the_30_hz_stream():
    """The gate publishes while round(pub_count / elapsed) <= FREQ, i.e. while the rate since the last reset of the control is below
    FREQ + 0.5, and resets the control when the rate is within 1 % of FREQ: over a long stretch the published rate lies in
    [0.99 FREQ - 1 / T, FREQ + 0.5 + 1 / T] for a stretch of T seconds (one message more or less at either end)."""
    freq, hz, n = 10, 30, 900
    st = stream(hz, n, start=200.0)
    w = restated(st, freq)
    t_pub = [t for t, (_, b, _) in zip(st, w) if b in (nr.FIRST_PUBLICATION, nr.PUBLISHED)]
    T = t_pub[-1] - t_pub[0]
    rate = (len(t_pub) - 1) / T
    assert T > 25.0 and 0.99 * freq - 1.0 / T <= rate <= freq + 0.5 + 1.0 / T, rate
    # and no window of one second holds more than FREQ + 0.5 rounded up plus one messages
    tp = np.array(t_pub)
    assert max(int(((tp >= a) & (tp < a + 1.0)).sum()) for a in tp) <= freq + 2
