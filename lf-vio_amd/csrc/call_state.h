// call_state.h — what of an optimization call is still in flight on a context, and the per-call plan.  Plain C++ (no HIP): the
// moves decide, lfvio_hip.hip acts on what they return (the pattern of linb_plan.h and tr_decide.h); tests/test_call_state.py walks
// every reachable state on the CPU.
//
// The protocol.  lfvio_batch_optimize_begin returns as soon as the state is in the mailbox (dev_types.h MailWord); the gated
// marginalization of the same graph — or a worker on its own stream (kernels_spec.h) — runs on behind it.  finish(), a chained
// upload, a device-chained upload, a reallocation or any other entry point then collects, joins or overtakes that work.
//
// State = phase x behind x workers.  16 of the 36 combinations are reachable (the walk lists them):
//
//   phase        IDLE          no call in flight, nothing to collect
//                EARLY_FIRST   begin() returned on the state flag of the FIRST graph: the graph's tail, its copy of
//                              {tail_state .. chain_err} into the pinned PendingBlock and the prior are still to come
//                EARLY_TAIL    ... of the tail graph (the window needed more passes than the first graph carried): no words follow
//                HELD          a reallocation collected the prior of the call in flight on the caller's behalf (lfvio_ctx::held)
//   behind       CLEAN         stream 0 has been waited for
//                UNSYNCED      finish() took the prior from the mailbox; the last microseconds of the graph are the next join's
//                PIPELINED     a device-chained upload went out behind the marginalization in flight: the stream holds work nobody
//                              has waited for, and nobody has to — the next begin() goes out behind it in stream order
//   workers      NO_WORKERS
//                STARTED       the workers' graphs were launched for the last call; its tail_state is on the device only
//                KNOWN         ... and is (or will be, once stream 0 is idle) in the PendingBlock: the first graph carried the tail
//
//   reachable:   IDLE x {CLEAN, UNSYNCED, PIPELINED} x {NO_WORKERS, STARTED, KNOWN}
//                EARLY_FIRST x CLEAN x {NO_WORKERS, KNOWN}     EARLY_FIRST x PIPELINED x NO_WORKERS
//                EARLY_TAIL x CLEAN x {NO_WORKERS, STARTED}    EARLY_TAIL x PIPELINED x NO_WORKERS
//                HELD x CLEAN x NO_WORKERS
//                (EARLY_* x PIPELINED: begin() behind a device-chained upload, which starts no workers.  EARLY_FIRST knows its workers'
//                tail_state, EARLY_TAIL never does.  IDLE x CLEAN with workers outstanding: a call that ended in an error behind its
//                first graph, or a tail graph whose flag never came.  Nothing is UNSYNCED while a call is in flight.)
//   transient:   HELD x {UNSYNCED, PIPELINED} x any, inside reserve() only: between prior_held() — finish() has just taken the prior
//                from the mailbox — and the join() on the next line, which leaves HELD x CLEAN x NO_WORKERS.  The walk looks at
//                states where an entry point returns and does not see them; join() treats HELD as IDLE.
//
// Events (the moves below, one each) and what every entry point waits for:
//
//   entry point                         move(s)                              waits for
//   every entry point that touches      join()                               DRAIN: stream 0, then the workers' echo (wait_side);
//   the slots or stream 0                                                    READ_FIRST_WORDS: + the first graph's PendingBlock words.
//                                                                            Nothing when IDLE / HELD x CLEAN
//   lfvio_batch_optimize_begin          join(OVERTAKE_PIPELINED)             as above, but nothing when IDLE x PIPELINED
//   optimize (all forms)                optimize_started, loop_started,      the loop, chunk by chunk (synchronous), or the state flag
//                                       workers_started, first_graph_ended,  (begin).  The chain error is looked at where
//                                       loop_ended | early_from_first |      CHECK_CHAIN_ERR is returned and never by a join
//                                       early_from_tail
//   lfvio_batch_optimize_finish         held_handed_out | prior_from_mailbox the prior flag; else join() + stream 0
//   lfvio_batch_upload_chained          (finish's, when collectable())       the prior of the call in flight, after packing
//   lfvio_batch_upload_chained_device   chained_on_device                    nothing (refused unless can_chain_on_device())
//   reallocation (reserve)              (finish's) prior_held, join,         everything
//                                       graphs_dropped
//   graph key change, debug switches    graphs_dropped                       stream 0 when anything is behind
//   lfvio_batch_sync                    join, take_workers                   everything: IDLE / HELD x CLEAN x NO_WORKERS after it
//
// Oddities the walk found, kept as they are:
//   * PIPELINED is sticky: upload_chained_device -> begin -> finish leaves it set, a second begin() on the same resident window
//     overtakes again (harmless: stream order) and runs without workers.
//   * loop_started() drops the previous call's workers without waiting for their echo when a join was overtaken or had nothing to
//     wait for: no hit is counted and the ticket word is not cleared (it is rewritten two lines later).
//   * worker_wait_timed_out(): the context is left as after a successful wait, but the ticket word stays and the first graph's words
//     are not read.
#pragma once
#ifndef CALL_STATE_ASSERT  // (the walk of tests/test_call_state.py records a failed precondition instead of aborting)
#include <cassert>
#define CALL_STATE_ASSERT(x) assert(x)
#endif

// What one call of the optimization does, decided once where the call enters (batch_optimize_impl, lfvio_solve, lfvio_marginalize)
struct CallPlan {
  static constexpr int NO_MARG = -1;
  int count = 1;            // slots [0, count)
  int marg_flag = NO_MARG;  // LFVIO_MARGIN_OLD / _SECOND_NEW, or none (lfvio_solve)
  bool adaptive = true;     // the host watches the loop chunk by chunk (false: one static graph, lfvio_batch_optimize_async)
  bool fused = false;       // the gated gauge fix + marginalization ride in the loop's first graph (adaptive, with graphs, with a flag)
  bool early = false;       // return on the state flag (lfvio_batch_optimize_begin)
  bool publish = false;     // the gated gauge fix and the marginalization push state and prior into the mailbox: a kernel argument and
                            // a graph index, so the plain call pays nothing for the split one
  int max_iter = 0;         // the largest max_num_iterations of the slots
  double max_seconds = -1;  // the smallest positive max_solver_time_in_seconds (<= 0: no cap; adaptive only)
};

struct CallState {
  enum Phase { IDLE, EARLY_FIRST, EARLY_TAIL, HELD };
  enum Behind { CLEAN, UNSYNCED, PIPELINED };
  enum Workers { NO_WORKERS, STARTED, KNOWN };
  enum Act : unsigned {
    NOTHING = 0,
    DRAIN = 1,             // synchronize stream 0, then wait for the workers (take_workers)
    READ_FIRST_WORDS = 2,  // ... then take the counts and tail_state the first graph left in the PendingBlock
    FEED_PREDICTION = 4,   // the call's loop has ended: its pass count sizes the next first graph
    CHECK_CHAIN_ERR = 8,   // look at the chain-error word that has just arrived and report it
  };
  enum Overtake { WAIT, OVERTAKE_PIPELINED };

  Phase phase = IDLE;
  Behind behind = CLEAN;
  Workers workers = NO_WORKERS;
  int marg_flag = 0;  // of the last optimize: which of the resident window's two planned priors a device-chained upload takes over
  int ticket = 0;     // last ticket handed to workers (never 0)

  // ---- queries
  bool early() const { return phase == EARLY_FIRST || phase == EARLY_TAIL; }
  bool pending() const { return phase != IDLE; }  // lfvio_batch_optimize_pending: a prior is collectable (in flight or held)
  bool can_chain_on_device() const { return early(); }
  bool pipelined() const { return behind == PIPELINED; }
  bool workers_outstanding() const { return workers != NO_WORKERS; }
  // (after DRAIN's synchronization, before take_workers) the prior of the call in flight was a worker's
  bool handed_to_worker(bool tail_is_workers) const { return workers == KNOWN && tail_is_workers; }

  // ---- moves
  // First statement of everything that touches the slots or stream 0.
  unsigned join(Overtake o = WAIT) {
    if (o == OVERTAKE_PIPELINED && behind == PIPELINED && !early()) return NOTHING;
    if (behind == CLEAN && !early()) return NOTHING;
    const unsigned act = DRAIN | (phase == EARLY_FIRST ? READ_FIRST_WORDS : 0);
    behind = CLEAN;
    if (early()) phase = IDLE;
    return act;
  }
  // The wait for the workers begins: what is outstanding (KNOWN: tail_state is in the PendingBlock; STARTED: read it from the slot)
  Workers take_workers() {
    const Workers w = workers;
    workers = NO_WORKERS;
    return w;
  }
  void worker_wait_timed_out() { CALL_STATE_ASSERT(workers == NO_WORKERS); }  // (the oddity above: nothing is put back)
  // Graphs are about to be destroyed: true = synchronize stream 0 first.  (With a call in flight only from lfvio_destroy.)
  bool graphs_dropped() {
    const bool sync = early() || behind != CLEAN;
    behind = CLEAN;
    return sync;
  }
  // An optimization begins, behind its join: a held prior nobody collected is dropped, like one left in the slot
  void optimize_started(int flag) {
    CALL_STATE_ASSERT(!early() && (behind == CLEAN || behind == PIPELINED));
    if (phase == HELD) phase = IDLE;
    marg_flag = flag;
  }
  // The adaptive loop is about to launch its first graph.  Returns the ticket for the mailbox: a new one when workers go out, else 0
  int loop_started(bool with_workers) {
    CALL_STATE_ASSERT(!early() && !(with_workers && behind == PIPELINED));
    workers = NO_WORKERS;  // (the oddity above)
    return with_workers ? (ticket = ticket == 0x7fffffff ? 1 : ticket + 1) : 0;
  }
  void workers_started() {
    CALL_STATE_ASSERT(workers == NO_WORKERS);
    workers = STARTED;
  }
  // The first graph ran to its end under the host's eyes; closed: it carried the tail and the window was done inside it
  unsigned first_graph_ended(bool carried_tail, bool closed) {
    if (carried_tail && closed && workers == STARTED) workers = KNOWN;
    return carried_tail ? CHECK_CHAIN_ERR : NOTHING;
  }
  unsigned loop_ended() { return FEED_PREDICTION; }  // synchronous end of the loop (the tail graph may still follow)
  unsigned early_from_first() {
    CALL_STATE_ASSERT(phase == IDLE && behind != UNSYNCED);
    phase = EARLY_FIRST;
    if (workers == STARTED) workers = KNOWN;
    return FEED_PREDICTION | CHECK_CHAIN_ERR;
  }
  unsigned early_from_tail() {  // (loop_ended has fed the prediction)
    CALL_STATE_ASSERT(phase == IDLE && behind != UNSYNCED && workers != KNOWN);
    phase = EARLY_TAIL;
    return CHECK_CHAIN_ERR;
  }
  // finish() found the prior flag up: the prior is the mailbox's, what is left of the graph is the next join's
  void prior_from_mailbox() {
    CALL_STATE_ASSERT(early());
    phase = IDLE;
    if (behind == CLEAN) behind = UNSYNCED;
  }
  // The window uploaded takes the prior of the call in flight over on the device: nothing of that call is left to collect
  void chained_on_device() {
    CALL_STATE_ASSERT(can_chain_on_device());
    phase = IDLE, behind = PIPELINED;
  }
  // reserve(): finish() has just collected the prior of the call in flight into lfvio_ctx::held.  `behind` is whatever finish() left
  // (the transient states of the table): the caller joins next
  void prior_held() {
    CALL_STATE_ASSERT(phase == IDLE);
    phase = HELD;
  }
  bool held_handed_out() {  // finish(): true = the held prior is the answer (once)
    if (phase != HELD) return false;
    phase = IDLE;
    return true;
  }
};
