"""CPU walk of the context's memory rule (lf-vio_amd/csrc/dev_mem.h: Buf, the one owning grow-only buffer every allocation of
lfvio_ctx and lfvio_group is a member of).  The header is plain C++, compiled here alone with g++ into a small shared object and driven
through ctypes, like tests/test_call_state.py.  The allocator policy of the shim records every allocation and free in order and fails
the k-th allocation on request; `feat_reserve` and `mask_replace` restate, move for move, the two call sites whose order matters
(feat.inc: the paired device + pinned scratch; gft.inc: the base mask, new block first).

Asserted: (1) a reserve within capacity calls no allocator and keeps the pointer; (2) growth is free-then-allocate of exactly the bytes
asked for, and the capacity never shrinks; (3) a failed allocation leaves the buffer empty, frees nothing, and the next reserve
succeeds; (4) over construction, moves, move-assignment over a non-empty buffer, reset and destruction every block is freed exactly
once and none is left, and a failed replacement leaves the old block owned; (5) when the second allocation of the paired grow fails
both halves are empty, and a retry succeeds."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>
#include "dev_mem.h"
struct Event { long long op, tag, addr, bytes; };  // op 1: allocated, 2: allocation failed, 3: freed
static std::vector<Event> events;
static int allocs = 0, fail_at = 0;
template <int TAG> struct Rec {
  static void *alloc(size_t bytes) {
    void *p = ++allocs == fail_at ? nullptr : std::malloc(bytes ? bytes : 1);
    events.push_back({p ? 1 : 2, TAG, (long long)(uintptr_t)p, (long long)bytes});
    return p;
  }
  static bool free(void *p) {
    events.push_back({3, TAG, (long long)(uintptr_t)p, 0});
    std::free(p);
    return true;
  }
};
using D = Buf<char, Rec<0>>;
using H = Buf<char, Rec<1>>;
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
extern "C" {
void rec_start(int fail) { events.clear(), allocs = 0, fail_at = fail; }
int rec_events(long long *out, int cap) {
  for (size_t k = 0; k < events.size() && (int)k < cap; k++) out[4 * k] = events[k].op, out[4 * k + 1] = events[k].tag, out[4 * k + 2] = events[k].addr, out[4 * k + 3] = events[k].bytes;
  return (int)events.size();
}
D *d_new() { return new D; }
H *h_new() { return new H; }
void d_delete(D *b) { delete b; }
void h_delete(H *b) { delete b; }
int d_reserve(D *b, size_t bytes) { return b->reserve(bytes); }
int d_reset(D *b) { return b->reset(); }
uintptr_t d_ptr(D *b) { return (uintptr_t)b->get(); }
size_t d_cap(D *b) { return b->capacity(); }
uintptr_t h_ptr(H *b) { return (uintptr_t)b->get(); }
size_t h_cap(H *b) { return b->capacity(); }
int d_converts(D *b) { char *p = *b; return p == b->get() && (!p || p + 3 == *b + 3) && (bool)*b == (p != nullptr); }
D *d_move_new(D *b) { return new D(std::move(*b)); }
void d_move_assign(D *dst, D *src) { *dst = std::move(*src); }
// gft.inc, lfvio_gft_set_mask: the new block first, then (the stream synchronized) it replaces the old one
int mask_replace(D *mask, size_t n) {
  if (mask->capacity() < n) {
    D fresh;
    if (!fresh.reserve(n)) return -3;
    *mask = std::move(fresh);
  }
  return 0;
}
// feat.inc, feat_reserve
int feat_reserve(D *d_feat, H *h_feat, size_t bytes) {
  if (bytes <= h_feat->capacity()) return 0;
  (void)d_feat->reset(), (void)h_feat->reset();
  bytes = align_up(bytes + bytes / 4, 4096);
  if (!d_feat->reserve(bytes) || !h_feat->reserve(bytes)) {
    (void)d_feat->reset();
    return -3;
  }
  return 0;
}
}
'''
ALLOC, FAILED, FREE = 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="dev_mem_")
    src, so = os.path.join(d, "dm.cpp"), os.path.join(d, "libdm.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    for f in ("d_new", "h_new", "d_move_new"):
        getattr(so, f).restype = C.c_void_p
    for f in ("d_ptr", "h_ptr"):
        getattr(so, f).restype, getattr(so, f).argtypes = C.c_size_t, [C.c_void_p]
    for f in ("d_cap", "h_cap"):
        getattr(so, f).restype, getattr(so, f).argtypes = C.c_size_t, [C.c_void_p]
    for f in ("d_delete", "h_delete", "d_reset", "d_converts", "d_move_new"):
        getattr(so, f).argtypes = [C.c_void_p]
    so.d_delete.restype = so.h_delete.restype = so.d_move_assign.restype = None
    so.d_reserve.argtypes = so.mask_replace.argtypes = [C.c_void_p, C.c_size_t]
    so.d_move_assign.argtypes = [C.c_void_p, C.c_void_p]
    so.feat_reserve.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    so.rec_events.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    return so


def events(lib):
    buf = (C.c_longlong * (4 * 256))()
    n = lib.rec_events(buf, 256)
    assert n <= 256
    return [tuple(buf[4 * k:4 * k + 4]) for k in range(n)]


def live(ev):
    """the blocks still allocated after `ev`; asserts that only live blocks are freed (nothing twice, nothing foreign)"""
    held = {}
    for op, tag, addr, nbytes in ev:
        if op == ALLOC:
            assert addr and (tag, addr) not in held
            held[tag, addr] = nbytes
        elif op == FREE:
            assert (tag, addr) in held, "freed twice, or never allocated"
            del held[tag, addr]
    return held


def test_reserve_within_capacity_is_free_of_allocator_calls(lib):
    lib.rec_start(0)
    b = lib.d_new()
    assert lib.d_ptr(b) == 0 and lib.d_cap(b) == 0 and lib.d_converts(b)
    assert lib.d_reserve(b, 0) == 1 and events(lib) == []  # nothing asked of an empty buffer: nothing done
    assert lib.d_reserve(b, 4096) == 1
    p, before = lib.d_ptr(b), events(lib)
    assert p and lib.d_converts(b) and before == [(ALLOC, 0, p, 4096)]
    for n in (4096, 4095, 1, 0):
        assert lib.d_reserve(b, n) == 1 and lib.d_ptr(b) == p and lib.d_cap(b) == 4096
    assert events(lib) == before
    lib.d_delete(b)
    assert events(lib) == before + [(FREE, 0, p, 0)]


def test_growth_frees_first_and_allocates_exactly(lib):
    lib.rec_start(0)
    b = lib.d_new()
    cap, expect = 0, []
    for n in (64, 16, 4096, 4096, 100, 1 << 20):
        old = lib.d_ptr(b)
        assert lib.d_reserve(b, n) == 1
        if n > cap:  # the old block goes BEFORE the new one comes: peak memory does not rise
            expect += ([(FREE, 0, old, 0)] if old else []) + [(ALLOC, 0, lib.d_ptr(b), n)]
            cap = n
        else:
            assert lib.d_ptr(b) == old
        assert lib.d_cap(b) == cap and events(lib) == expect
    assert len(live(events(lib))) == 1
    lib.d_delete(b)
    assert live(events(lib)) == {}


@pytest.mark.parametrize("first", [True, False])
def test_a_failed_allocation_leaves_an_empty_buffer_and_a_retry_succeeds(lib, first):
    lib.rec_start(1 if first else 2)
    b = lib.d_new()
    if not first:
        assert lib.d_reserve(b, 256) == 1
    old = lib.d_ptr(b)
    assert lib.d_reserve(b, 1000) == 0
    assert lib.d_ptr(b) == 0 and lib.d_cap(b) == 0 and lib.d_converts(b)
    ev = events(lib)
    assert ev[-1] == (FAILED, 0, 0, 1000)
    # the old block went before the attempt, as in every growth; the failed attempt itself frees nothing
    assert [e for e in ev if e[0] == FREE] == ([] if first else [(FREE, 0, old, 0)]) and live(ev) == {}
    assert lib.d_reserve(b, 1000) == 1 and lib.d_ptr(b) and lib.d_cap(b) == 1000
    assert events(lib) == ev + [(ALLOC, 0, lib.d_ptr(b), 1000)]
    assert lib.d_reset(b) == 1 and lib.d_ptr(b) == 0 and lib.d_cap(b) == 0
    assert lib.d_reset(b) == 1  # an empty buffer: nothing to free
    lib.d_delete(b)
    assert live(events(lib)) == {} and len(events(lib)) == len(ev) + 2


def test_every_block_is_freed_exactly_once(lib):
    lib.rec_start(0)
    a = lib.d_new()
    assert lib.d_reserve(a, 100) == 1
    pa = lib.d_ptr(a)
    b = lib.d_move_new(a)  # move construction: the block changes hands, the source is empty
    assert (lib.d_ptr(b), lib.d_cap(b), lib.d_ptr(a), lib.d_cap(a)) == (pa, 100, 0, 0) and len(events(lib)) == 1
    assert lib.d_reserve(a, 200) == 1  # a moved-from buffer is an empty buffer
    pa2 = lib.d_ptr(a)
    lib.d_move_assign(b, a)  # over a non-empty buffer: its block is freed, the other's taken
    assert (lib.d_ptr(b), lib.d_cap(b), lib.d_ptr(a), lib.d_cap(a)) == (pa2, 200, 0, 0)
    assert events(lib)[-1] == (FREE, 0, pa, 0) and live(events(lib)) == {(0, pa2): 200}
    lib.d_move_assign(b, b)  # onto itself: nothing
    assert lib.d_ptr(b) == pa2 and live(events(lib)) == {(0, pa2): 200}
    lib.d_move_assign(b, a)  # from an empty buffer: b is empty too
    assert lib.d_ptr(b) == 0 and lib.d_cap(b) == 0 and live(events(lib)) == {}
    assert lib.d_reserve(b, 300) == 1 and lib.d_reset(b) == 1 and live(events(lib)) == {}
    assert lib.d_reserve(b, 50) == 1
    lib.d_delete(a), lib.d_delete(b)  # an empty one and a full one
    ev = events(lib)
    assert live(ev) == {} and sum(e[0] == ALLOC for e in ev) == sum(e[0] == FREE for e in ev) == 4


def test_the_mask_is_replaced_only_by_a_block_that_exists(lib):
    lib.rec_start(3)  # the third allocation fails
    m = lib.d_new()
    assert lib.mask_replace(m, 1000) == 0
    p1 = lib.d_ptr(m)
    assert lib.mask_replace(m, 900) == 0 and lib.d_ptr(m) == p1 and len(events(lib)) == 1  # fits
    assert lib.mask_replace(m, 2000) == 0
    p2, ev = lib.d_ptr(m), events(lib)
    assert ev[1:] == [(ALLOC, 0, p2, 2000), (FREE, 0, p1, 0)] and lib.d_cap(m) == 2000  # the new block FIRST
    assert lib.mask_replace(m, 3000) == -3  # refused: the old mask stays, owned and unchanged
    assert lib.d_ptr(m) == p2 and lib.d_cap(m) == 2000
    assert events(lib) == ev + [(FAILED, 0, 0, 3000)] and live(events(lib)) == {(0, p2): 2000}
    assert lib.mask_replace(m, 3000) == 0 and lib.d_cap(m) == 3000
    lib.d_delete(m)
    assert live(events(lib)) == {}


@pytest.mark.parametrize("fail", [0, 1, 2, 3, 4])
def test_the_paired_scratch_grows_as_one(lib, fail):
    lib.rec_start(fail)
    d, h = lib.d_new(), lib.h_new()
    sizes = lambda: (lib.d_cap(d), lib.h_cap(h))
    want = lambda n: (n + n // 4 + 4095) // 4096 * 4096
    rc = lib.feat_reserve(d, h, 1000)
    if fail in (1, 2):  # the device half, or the pinned half behind it: neither is left
        assert rc == -3 and sizes() == (0, 0) and lib.d_ptr(d) == 0 and lib.h_ptr(h) == 0 and live(events(lib)) == {}
        assert lib.feat_reserve(d, h, 1000) == 0  # a retry allocates both
    else:
        assert rc == 0
    assert sizes() == (want(1000),) * 2 and lib.d_ptr(d) and lib.h_ptr(h)
    n = len(events(lib))
    assert lib.feat_reserve(d, h, want(1000)) == 0 and len(events(lib)) == n  # inside the headroom
    rc = lib.feat_reserve(d, h, 100000)
    if fail in (3, 4):
        assert rc == -3 and sizes() == (0, 0) and live(events(lib)) == {}
        rc = lib.feat_reserve(d, h, 100000)
    assert rc == 0 and sizes() == (want(100000),) * 2
    ev = events(lib)
    assert [e[1] for e in ev[n:n + 2]] == [0, 1] and all(e[0] == FREE for e in ev[n:n + 2])  # both old halves go before either new one comes
    assert sorted(live(ev).values()) == [want(100000)] * 2 and {t for t, _ in live(ev)} == {0, 1}
    lib.d_delete(d), lib.h_delete(h)
    assert live(events(lib)) == {}
