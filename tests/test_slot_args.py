"""CPU walk of the kernels' argument offsets (lf-vio_amd/csrc/slot_args.h: SlotArgs, built per context from Layout).  The header is plain
C++, compiled here with g++ into a small shared object and driven through ctypes, like tests/test_call_state.py.

k_lin and k_spec_begin take the byte offsets of the arrays they read first as a kernel argument and issue those loads together with the
slot header's — before the header has said how large the window is.  Such a load is speculative: its index is clamped into the array's
capacity by the first_*_index() functions of the header, which the kernels call.  slot_arg_spans() derives, per offset, how many bytes those
first-round loads can reach from the SAME functions at the largest index there is, and states next to it the bytes Layout gave the array.
Asserted here, for capacities from an empty context to one just past SPEC_MAX_LM, with and without the shadow slots of a one-window context:

  (a) offset + reach lies inside [0, Layout::total) of the slot the offset is meant for, and the reach inside the array's own bytes, for
      every offset — a clamp against another array's capacity (cap_lm where cap_lm_in is needed) fails here;
  (b) the shadow variant's input offsets land in slot 0's blob (and are the plain variant's moved back by the shadow's distance), its
      work-array offsets stay in the shadow's own blob;
  (c) the prior role's speculative rounds of J0 cover a staged prior (76 rows) and stay inside the array whatever the prior's size (0, 76);
  (d) no two arrays' first-round reaches overlap: a reach that ran past its own array would run into the next one."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "slot_args.h"
extern "C" int sa_count() { return SLOT_ARG_SPANS; }
extern "C" int sa_first_prior_j() { return FIRST_PRIOR_J; }
extern "C" int sa_input_offsets() { return SLOT_INPUT_OFFSETS; }
extern "C" long long sa_prior_j_bytes() { return (long long)LFVIO_MAX_PRIOR_DIM * LFVIO_MAX_PRIOR_DIM * 8; }
// back_slots: 0 the slot's own variant; k > 0: the variant of a shadow slot k slots behind slot 0
extern "C" long long sa_walk(int maxN, int maxM, int back_slots, const char **name, long long *off, long long *bytes, long long *array, int *input, long long *raw, int *caps) {
  const Layout L = make_layout(maxN, maxM);
  const SlotArgs A = slot_args(L, (size_t)back_slots * L.total);
  SlotArgSpan sp[SLOT_ARG_SPANS + 8];
  const int n = slot_arg_spans(L, A, sp);
  if (n != SLOT_ARG_SPANS) return -1;
  for (int k = 0; k < n; k++) name[k] = sp[k].name, off[k] = sp[k].off, bytes[k] = sp[k].bytes, array[k] = sp[k].array, input[k] = sp[k].input;
  static_assert(sizeof(SlotArgs) % 8 == 0, "whole words");
  const long long *w = (const long long *)&A;
  for (int k = 0; k < SLOT_INPUT_OFFSETS; k++) raw[k] = w[k];
  caps[0] = A.cap_lm_in, caps[1] = A.cap_chunks, caps[2] = A.cap_blocks, caps[3] = A.cap_lm;
  // the index functions the kernels call, at indices far past any window: inside the capacity they are meant for
  if (first_lm_in_index(A, 1 << 30) != A.cap_lm_in - 1 || first_chunk_index(A, 1 << 30) != A.cap_chunks - 1 || first_lm_index(A, 1 << 30) != A.cap_lm - 1) return -2;
  if (first_block_index(A.cap_blocks, 63) > A.cap_blocks - 1 || first_blockE_index(A.cap_blocks, 63) > SPEC_MAX_LM / 64 - 1) return -3;
  if (first_lm_in_index(A, 0) != 0 || first_lm_index(A, 0) != 0 || first_chunk_index(A, 0) != 0 || first_block_index(A.cap_blocks, 0) != 0) return -4;
  return (long long)L.total;
}
'''
CAPACITIES = (0, 1, 24, 33, 300, 320, 321)
ARRAY = {}  # (maxN, maxM) -> array name -> bytes Layout gave it
WORKERS = 2  # shadow slots of a one-window context (lfvio_ctx::WORKERS)


def max_m(n, per):
    return n * per


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="slot_args_")
    src, so = os.path.join(d, "sa.cpp"), os.path.join(d, "libsa.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.sa_walk.restype = C.c_longlong
    so.sa_prior_j_bytes.restype = C.c_longlong
    return so


def walk(lib, n, m, back):
    cnt = lib.sa_count()
    name, off, nbytes, arr, inp = (C.c_char_p * cnt)(), (C.c_longlong * cnt)(), (C.c_longlong * cnt)(), (C.c_longlong * cnt)(), (C.c_int * cnt)()
    raw, caps = (C.c_longlong * lib.sa_input_offsets())(), (C.c_int * 4)()
    total = lib.sa_walk(n, m, back, name, off, nbytes, arr, inp, raw, caps)
    assert total > 0, total
    ARRAY[n, m] = {name[k].decode(): arr[k] for k in range(cnt)}
    spans = [(name[k].decode(), off[k], nbytes[k], bool(inp[k])) for k in range(cnt)]
    return total, spans, list(raw), list(caps)


CASES = [(n, max_m(n, per)) for n in CAPACITIES for per in ((0,) if n == 0 else (1, 4, 11))]


@pytest.mark.parametrize("n,m", CASES)
def test_first_round_reaches_stay_inside_the_blob(lib, n, m):
    total, spans, _, caps = walk(lib, n, m, 0)
    assert all(c >= 1 for c in caps), caps  # a clamp needs an entry to clamp to
    assert caps[3] >= 64 and caps[3] % 64 == 0
    for name, off, nbytes, _ in spans:
        assert nbytes >= 4, name
        assert 0 <= off and off + nbytes <= total, (name, off, nbytes, total)  # (a)
        assert nbytes <= ARRAY[n, m][name], (name, nbytes, ARRAY[n, m][name])
    # (d) sorted by offset, a reach ends before the next array begins
    by_off = sorted(spans, key=lambda s: s[1])
    for (na, oa, ba, _), (nb, ob, _, _) in zip(by_off, by_off[1:]):
        assert oa + ba <= ob, (na, oa, ba, nb, ob)


@pytest.mark.parametrize("n,m", CASES)
@pytest.mark.parametrize("back", range(1, 1 + WORKERS))
def test_shadow_inputs_lead_into_slot_zero(lib, n, m, back):
    total, own, raw_own, _ = walk(lib, n, m, 0)
    total2, shadow, raw_shadow, _ = walk(lib, n, m, back)
    assert total2 == total
    dist = back * total
    n_in = 0
    for (name, off, nbytes, inp), (name_s, off_s, nbytes_s, inp_s) in zip(own, shadow):
        assert (name, nbytes, inp) == (name_s, nbytes_s, inp_s)
        if inp:  # (b) from the shadow's header: into slot 0's blob, at the same place as slot 0's own
            n_in += 1
            assert off_s == off - dist, name
            assert 0 <= off_s + dist and off_s + dist + nbytes <= total, (name, off_s, nbytes)
        else:
            assert off_s == off, name
            assert 0 <= off_s and off_s + nbytes <= total, (name, off_s, nbytes)
    assert n_in >= 10
    # every input member of the struct but the stride between the observation channels moves back
    moved = [a - b for a, b in zip(raw_own, raw_shadow)]
    assert sorted(set(moved)) == [0, dist] and moved.count(0) == 1, moved


@pytest.mark.parametrize("prior_n", (0, 76))
def test_prior_rounds(lib, prior_n):
    # (c) k_lin's prior role asks for FIRST_PRIOR_J entries of J0 whatever the prior's size; a staged prior (<= 76 rows) is covered
    first = lib.sa_first_prior_j()
    assert first % 256 == 0 and prior_n * prior_n <= first and first * 8 <= lib.sa_prior_j_bytes()
    for n, m in CASES:
        total, spans, _, _ = walk(lib, n, m, 0)
        (off, nbytes), = [(o, b) for nm, o, b, _ in spans if nm == "prior_J"]
        assert nbytes == first * 8 and off + nbytes <= total

