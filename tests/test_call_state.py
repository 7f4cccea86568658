"""CPU walk of the host's call state (lf-vio_amd/csrc/call_state.h: what of a split optimization call is still in flight, and what
every entry point has to wait for).  The header is plain C++, compiled here with g++ into a small shared object and driven through
ctypes, like tests/test_linb_plan.py.  `Driver` below restates, move for move, how lfvio_hip.hip uses the header at each entry point;
the walk is breadth-first over ALL states reachable under all entry points and all values of the device words a move depends on
(tail_state 0 / 2 / 3, chain error 0 / 1, the worker's echo, the two mailbox flags, whether the window closes inside its first graph).

Asserted: (a) the reachable set is the table of the header; (b) after lfvio_batch_sync — the full join — nothing is in flight and no
workers are outstanding; (c) a join answers "nothing to wait for" only when idle, or for begin() behind a device-chained upload;
(d) every adaptive call that ends feeds the pass prediction exactly once; (e) a chain error is reported once per call and never by a
join; (f) pending() is true exactly while a prior is collectable; (g) a device-chained upload is accepted only from "early, nothing
held"; (h) a held prior is handed out once and dropped by the next optimize; (i) no precondition of a move fails on a reachable path."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile
from collections import deque, namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
static const char *failed = nullptr;
#define CALL_STATE_ASSERT(x) ((x) ? (void)0 : (void)(failed = #x))
#include "call_state.h"
extern "C" int cs_move(int state, int move, int a, int b, unsigned *out, const char **why) {
  CallState s;
  s.phase = CallState::Phase(state & 3), s.behind = CallState::Behind(state >> 2 & 3), s.workers = CallState::Workers(state >> 4 & 3);
  failed = nullptr;
  unsigned r = 0;
  switch (move) {
    case 0: r = s.join(a ? CallState::OVERTAKE_PIPELINED : CallState::WAIT); break;
    case 1: r = s.take_workers(); break;
    case 2: s.worker_wait_timed_out(); break;
    case 3: r = s.graphs_dropped(); break;
    case 4: s.optimize_started(a); break;
    case 5: r = s.loop_started(a != 0) != 0; break;
    case 6: s.workers_started(); break;
    case 7: r = s.first_graph_ended(a != 0, b != 0); break;
    case 8: r = s.loop_ended(); break;
    case 9: r = s.early_from_first(); break;
    case 10: r = s.early_from_tail(); break;
    case 11: s.prior_from_mailbox(); break;
    case 12: s.chained_on_device(); break;
    case 13: s.prior_held(); break;
    case 14: r = s.held_handed_out(); break;
    default: r = s.early() | s.pending() << 1 | s.can_chain_on_device() << 2 | s.pipelined() << 3 | s.workers_outstanding() << 4 | s.handed_to_worker(a != 0) << 5;
  }
  *out = r, *why = failed;
  return s.phase | s.behind << 2 | s.workers << 4;
}
'''
MOVES = ("join take_workers worker_wait_timed_out graphs_dropped optimize_started loop_started workers_started first_graph_ended "
         "loop_ended early_from_first early_from_tail prior_from_mailbox chained_on_device prior_held held_handed_out query").split()
DRAIN, READ_FIRST_WORDS, FEED_PREDICTION, CHECK_CHAIN_ERR = 1, 2, 4, 8
PHASE, BEHIND, WORKERS = ("IDLE", "EARLY_FIRST", "EARLY_TAIL", "HELD"), ("CLEAN", "UNSYNCED", "PIPELINED"), ("NO_WORKERS", "STARTED", "KNOWN")
TAIL_OPEN, TAIL_DONE, TAIL_WORKER = 0, 2, 3
OK, ERR = 0, 1


def name(state):
    return PHASE[state & 3], BEHIND[state >> 2 & 3], WORKERS[state >> 4 & 3]


# the header's table
REACHABLE = {("IDLE", b, w) for b in BEHIND for w in WORKERS} | {
    ("EARLY_FIRST", "CLEAN", "NO_WORKERS"), ("EARLY_FIRST", "CLEAN", "KNOWN"), ("EARLY_FIRST", "PIPELINED", "NO_WORKERS"),
    ("EARLY_TAIL", "CLEAN", "NO_WORKERS"), ("EARLY_TAIL", "CLEAN", "STARTED"), ("EARLY_TAIL", "PIPELINED", "NO_WORKERS"), ("HELD", "CLEAN", "NO_WORKERS")}

# The device words an entry point may meet.  ts: Slot::tail_state as the host reads it; echo: the worker's echo of the ticket is there;
# closes: the window is done inside its first graph; state_flag / prior_flag: the mailbox flag arrives before stream 0 is idle
World = namedtuple("World", "ts echo chain_err closes state_flag prior_flag workers_ok mailbox new_key")
VALUES = dict(ts=(TAIL_OPEN, TAIL_DONE, TAIL_WORKER))  # every other word: 0 / 1


def worlds(fields):
    """every value of the words an entry point looks at, the others 0"""
    return [World(**{**dict.fromkeys(World._fields, 0), **dict(zip(fields, v))}) for v in itertools.product(*[VALUES.get(f, (0, 1)) for f in fields])]


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="call_state_")
    src, so = os.path.join(d, "cs.cpp"), os.path.join(d, "libcs.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lf-vio_amd", "csrc"), src, "-o", so])
    so = C.CDLL(so)
    so.cs_move.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_char_p)]
    return so


class Driver:
    """lfvio_hip.hip's use of CallState, entry point by entry point.  log: what the host does that a caller or the device can see."""

    def __init__(self, lib, state=0):
        self.lib, self.state, self.log, self.failed = lib, state, [], []

    def move(self, what, a=0, b=0):
        out, why = C.c_uint(0), C.c_char_p()
        self.state = self.lib.cs_move(self.state, MOVES.index(what), int(a), int(b), C.byref(out), C.byref(why))
        if why.value:
            self.failed.append((what, why.value.decode()))
        return out.value

    def q(self, bit, a=0):
        return bool(self.move("query", a) >> bit & 1)

    early = lambda self: self.q(0)
    pending = lambda self: self.q(1)

    # ---- join_inflight, wait_side
    def wait_side(self, w):
        k = self.move("take_workers")
        if k == 0:
            return OK
        self.log.append("tail_state from " + ("the pinned block" if WORKERS[k] == "KNOWN" else "the slot"))
        if w.ts == TAIL_WORKER and not w.echo:
            self.move("worker_wait_timed_out")
            self.log.append("error: worker timeout")
            return ERR
        self.log += ["hit"] * w.echo + ["ticket word cleared"]
        return OK

    def join(self, w, overtake=False):
        before = name(self.state)
        act = self.move("join", overtake)
        if not act & DRAIN:
            self.log.append("nothing to wait for")
            assert before[0] in ("IDLE", "HELD") and (before[1] == "CLEAN" or (overtake and before[:2] == ("IDLE", "PIPELINED"))), before  # (c)
            return OK
        self.log.append("synchronize stream 0")
        handed = self.q(5, w.ts == TAIL_WORKER)
        if self.wait_side(w):
            return ERR
        if act & READ_FIRST_WORDS:
            self.log.append("first graph's words read")
            if w.ts != TAIL_DONE and not handed:
                self.log.append("error: marginalization did not finish")
                return ERR
        assert not act & (FEED_PREDICTION | CHECK_CHAIN_ERR)  # (d), (e): never a join
        return OK

    def drop_graphs(self):
        if self.move("graphs_dropped"):
            self.log.append("synchronize stream 0")

    # ---- entry points
    def finish(self, w, prior=True):
        if self.move("held_handed_out"):
            self.log.append("held prior handed out")
            return OK
        if self.early() and prior and w.prior_flag:
            self.move("prior_from_mailbox")
            self.log.append("prior from the mailbox")
            return OK
        if self.join(w):
            return ERR
        self.log.append("synchronize stream 0")
        if prior:
            self.log.append("prior downloaded")
        return OK

    def upload(self, w, kind="plain"):
        if kind == "device":
            if not self.q(2):
                self.log.append("refused")
                return ERR
        chained = kind == "chained" and self.pending()
        if kind == "plain" or (kind == "chained" and not chained):
            if self.join(w):
                return ERR
        if chained and self.finish(w):
            return ERR
        if self.q(4):
            self.log.append("k_spec_wait")
        if kind == "device":
            self.move("chained_on_device")
        self.log.append("uploaded")
        return OK

    def reserve_grow(self, w):
        if self.early():
            if self.finish(w):
                return ERR
            self.move("prior_held")
        if self.join(w):
            return ERR
        self.drop_graphs()
        return OK

    def sync(self, w):
        if self.join(w):
            return ERR
        self.log.append("synchronize stream 0")
        return self.wait_side(w)

    def configure(self, w):
        if self.join(w):
            return ERR
        self.drop_graphs()
        return OK

    def adaptive_loop(self, w, one, fused, begin, publish):
        if self.join(w, overtake=begin):
            return ERR, False
        if w.new_key:
            self.drop_graphs()
        ahead = fused and one and w.workers_ok and not self.q(3)
        ticket = self.move("loop_started", ahead)
        if one:
            self.log.append("ticket word: " + ("new" if ticket else "0"))
        if ahead:
            self.move("workers_started")
            self.log.append("workers launched")
        if begin and fused and publish and w.closes and w.state_flag:
            self.acts.append(self.move("early_from_first"))
            return OK, True
        act = self.move("first_graph_ended", fused and one, w.closes)
        self.acts.append(act)
        if act & CHECK_CHAIN_ERR and w.chain_err:
            self.log.append("error: chain")
            self.reports += 1
            return ERR, False
        self.acts.append(self.move("loop_ended"))
        if fused and w.closes and self.wait_side(w):
            return ERR, False
        return OK, fused and w.closes

    def optimize(self, w, form, one=True):
        """form: async | sync | begin | solve (lfvio_solve: no marginalization)"""
        self.acts, self.reports = [], 0
        begin = form == "begin"
        if form == "solve":
            rc = self.upload(w) or self.adaptive_loop(w, True, False, False, False)[0] or self.join(w)
        else:
            if self.join(w, overtake=begin and one):
                return ERR
            self.move("optimize_started")
            publish = begin and one and w.mailbox
            if form == "async":
                return self.join(w) or self.join(w)  # (enqueue_solve's, enqueue_marg's)
            rc, tail_done = self.adaptive_loop(w, one, True, begin, publish)
            if not rc and not tail_done:
                assert self.move("join", True) == 0  # (the gated marginalization's join inside the capture of the tail graph)
                if publish and w.state_flag:
                    self.acts.append(self.move("early_from_tail"))
            if not rc and form == "sync":
                rc = self.sync(w)
            if not rc and begin:
                if self.early():
                    assert self.acts[-1] & CHECK_CHAIN_ERR
                    if w.chain_err:
                        self.log.append("error: chain")
                        self.reports += 1
                        rc = ERR
                else:
                    rc = self.join(w)  # (download)
        if not rc:
            assert sum(bool(a & FEED_PREDICTION) for a in self.acts) == 1, self.acts  # (d)
        assert self.reports == (1 if w.chain_err and any(a & CHECK_CHAIN_ERR for a in self.acts) else 0)  # (e)
        return rc


def events():
    """name -> ((Driver, World) -> return code, its worlds); every entry point in every form"""
    join, collect = worlds(("ts", "echo")), worlds(("ts", "echo", "prior_flag"))
    call = worlds(("ts", "echo", "chain_err", "closes", "state_flag", "workers_ok", "mailbox", "new_key"))
    ev = {"upload": (lambda d, w: d.upload(w), join), "upload_chained": (lambda d, w: d.upload(w, "chained"), collect),
          "upload_chained_device": (lambda d, w: d.upload(w, "device"), join), "finish": (lambda d, w: d.finish(w), collect),
          "finish(no prior)": (lambda d, w: d.finish(w, prior=False), collect), "reserve": (Driver.reserve_grow, collect), "sync": (Driver.sync, join),
          "configure": (Driver.configure, join)}
    for form in ("async", "sync", "begin", "solve"):
        ev["optimize " + form] = (lambda d, w, form=form: d.optimize(w, form), call)
    for form in ("async", "sync", "begin"):
        ev["optimize " + form + " (batch)"] = (lambda d, w, form=form: d.optimize(w, form, one=False), call)
    return ev


def walk(lib, visit):
    """visit(state, event name, world, driver after the event, return code) for every edge; returns the reachable set"""
    seen, todo = {0}, deque([0])
    ev = events()
    while todo:
        s = todo.popleft()
        for nm, (run, ws) in ev.items():
            for w in ws:
                d = Driver(lib, s)
                rc = run(d, w)
                visit(s, nm, w, d, rc)
                if d.state not in seen:
                    seen.add(d.state)
                    todo.append(d.state)
    return seen


def test_the_reachable_states_are_the_table_and_no_precondition_fails(lib):
    def visit(s, nm, w, d, rc):
        assert not d.failed, (name(s), nm, w, d.failed)  # (i)
        assert d.pending() == (name(d.state)[0] != "IDLE")
    seen = walk(lib, visit)
    assert {name(s) for s in seen} == REACHABLE  # (a)


def test_joins_and_what_they_leave(lib):
    def visit(s, nm, w, d, rc):
        after = name(d.state)
        if nm == "sync" and rc == OK:
            assert after[0] in ("IDLE", "HELD") and after[1:] == ("CLEAN", "NO_WORKERS"), (name(s), w, after)  # (b)
        if nm == "upload_chained_device":  # (g)
            assert (rc == OK) == (name(s)[0] in ("EARLY_FIRST", "EARLY_TAIL")), (name(s), rc)
            assert after[:2] == (("IDLE", "PIPELINED") if rc == OK else name(s)[:2])
    walk(lib, visit)


def test_what_a_join_and_the_hand_over_moves_do_in_every_state(lib):
    """The header's "waits for" column, state by state: (state, overtake) -> (actions, next state) of join(), and the moves that decide
    what the next join has to wait for.  Over the reachable states and the transient ones inside reserve()."""
    transient = {("HELD", b, w) for b in ("UNSYNCED", "PIPELINED") for w in WORKERS}
    for phase, behind, workers in sorted(REACHABLE | transient):
        start = PHASE.index(phase) | BEHIND.index(behind) << 2 | WORKERS.index(workers) << 4
        for overtake in (False, True):
            if phase in ("IDLE", "HELD") and (behind == "CLEAN" or (overtake and behind == "PIPELINED")):
                want = (0, (phase, behind, workers))  # nothing to wait for, nothing changes
            else:  # the workers stay for take_workers(); only the first graph leaves words to read
                want = (DRAIN | (READ_FIRST_WORDS if phase == "EARLY_FIRST" else 0), ("HELD" if phase == "HELD" else "IDLE", "CLEAN", workers))
            d = Driver(lib, start)
            assert (d.move("join", overtake), name(d.state)) == want and not d.failed, (phase, behind, workers, overtake)
        if phase in ("EARLY_FIRST", "EARLY_TAIL"):
            d = Driver(lib, start)
            d.move("prior_from_mailbox")  # PIPELINED is sticky: only a clean stream becomes UNSYNCED
            assert name(d.state) == ("IDLE", "PIPELINED" if behind == "PIPELINED" else "UNSYNCED", workers) and not d.failed
            d = Driver(lib, start)
            d.move("chained_on_device")  # (the workers stay: the upload puts k_spec_wait in front of its copies)
            assert name(d.state) == ("IDLE", "PIPELINED", workers) and not d.failed
        d = Driver(lib, start)
        assert d.move("graphs_dropped") == (phase in ("EARLY_FIRST", "EARLY_TAIL") or behind != "CLEAN") and name(d.state) == (phase, "CLEAN", workers)
        d = Driver(lib, start)
        assert d.move("take_workers") == WORKERS.index(workers) and name(d.state) == (phase, behind, "NO_WORKERS")


def test_a_prior_is_pending_exactly_while_it_is_collectable(lib):
    """(f), (h): `collectable` is kept here from what the entry points did, not from the state"""
    seen, todo = {(0, False)}, deque([(0, False)])
    ev = events()
    while todo:
        s, collectable = todo.popleft()
        for nm, (run, ws) in ev.items():
            for w in ws:
                d = Driver(lib, s)
                rc = run(d, w)
                text = " ".join(d.log)
                c = collectable
                if nm.startswith("optimize") and nm != "optimize solve":  # (lfvio_solve is an upload and a loop of its own: a held prior stays)
                    c = d.early()  # a new call: whatever was there is dropped (h); collectable again iff it returned early
                    assert "held prior handed out" not in text
                elif "held prior handed out" in text or "prior from the mailbox" in text or "prior downloaded" in text:
                    assert text.count("held prior handed out") <= 1
                    c = nm == "reserve"  # (collected on the caller's behalf: held)
                    if "held prior handed out" in text:
                        assert name(s)[0] == "HELD" and name(d.state)[0] == "IDLE"  # (h): once
                elif "synchronize stream 0" in text and name(s)[0] != "HELD":
                    c = False  # joined: the prior stays in the slot (lfvio_batch_download), nothing is pending
                elif nm == "upload_chained_device" and rc == OK:
                    c = False  # taken over on the device
                if nm == "reserve" and name(s)[0] in ("EARLY_FIRST", "EARLY_TAIL") and rc != OK and "worker timeout" in text:
                    # the reallocation gave up half-way.  The prior had come through the mailbox and is held: collectable; or
                    # the timeout struck while finish() was joining for it: nothing was collected, nothing is pending
                    c = "prior from the mailbox" in text
                assert d.pending() == c, (name(s), collectable, nm, w, d.log, name(d.state))
                if (d.state, c) not in seen:
                    seen.add((d.state, c))
                    todo.append((d.state, c))
