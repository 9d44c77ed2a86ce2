// agent.cpp -- the host side of the two kernels that LINGER: the receive agent (sched.hip p2p_agent_kernel), which copies and
// acknowledges the blocking Receive's short messages (p2p.cpp), and the LL agent (ll.hip ll_agent_kernel), which runs a blocking
// small collective (dsync.cpp dsync_ll) -- either without a launch per call.  Compiled by hipcc as host code.
//
// Both are talked to over a record of 8 words in pinned host memory, with one protocol (tests/agent_sim.py models it):
//   [1] [2]  the command's two pointers, relaxed
//   [3]      what the command is about in the low half, its number in the high half, release
//   [0]      the doorbell, LAST: 1 = a command (| bytes << 2), 2 = stop; its number from bit 24 up; 0 = withdrawn, release
//   [6]      the agent's answer: the number of the command it has completed
//   [7]      != 0: the agent has gone (its patience ran out, or it was told to stop)
// The agent polls all four words while they are written and takes them only when [0] and [3] both carry this number: every word
// is an atomic store, so that the words it reads early are merely old, never torn.
#include <cstring>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

namespace {

constexpr int kWait = 2;  // a slow check's "nothing wrong yet" (the verdicts are 1 = answered, 0 = not taken, -1 = failed)

struct AgentLine {
  volatile uint64_t* cmd;
  uint64_t& seq;        // number of the last command written
  bool& running;        // launched and not yet known to have gone
  hipStream_t& stream;  // the agent's own: idle only when the agent has ended
  int device;

  bool answered(uint64_t n) const { return __atomic_load_n((const uint64_t*)&cmd[6], __ATOMIC_ACQUIRE) == n; }
  bool gone() const { return __atomic_load_n((const uint64_t*)&cmd[7], __ATOMIC_ACQUIRE) != 0; }

  // writes a command in protocol order and returns its number
  uint64_t post(uint64_t w1, uint64_t w2, uint64_t w3_low, size_t bytes) {
    const uint64_t n = ++seq;
    __atomic_store_n((uint64_t*)&cmd[1], w1, __ATOMIC_RELAXED);
    __atomic_store_n((uint64_t*)&cmd[2], w2, __ATOMIC_RELAXED);
    __atomic_store_n((uint64_t*)&cmd[3], w3_low | (n << 32), __ATOMIC_RELEASE);
    __atomic_store_n((uint64_t*)&cmd[0], 1ull | ((uint64_t)bytes << 2) | (n << 24), __ATOMIC_RELEASE);  // the doorbell last
    return n;
  }

  // The doorbell is withdrawn: nobody may act on it any more.  The number goes back only when nobody can have read the command
  // (no agent was there); otherwise it stays consumed and a relaunch starts at the next one.
  void withdraw(bool consume_number) {
    __atomic_store_n((uint64_t*)&cmd[0], 0, __ATOMIC_RELEASE);
    if (!consume_number) --seq;
  }

  // (re)starts the agent on its stream: launch_kernel(stream) -> hipError_t
  template <class Launch>
  bool start(Launch launch_kernel) {
    if (!stream) stream = stream_acquire(device);
    if (!stream) return false;
    __atomic_store_n((uint64_t*)&cmd[7], 0, __ATOMIC_RELEASE);
    if (launch_kernel(stream) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    running = true;
    return true;
  }

  // Waits for the answer to command n; an agent that had gone (its patience ran out) is started again.  Returns 1 = answered;
  // 0 = the agent could not be launched: the doorbell is withdrawn and the number given back (cannot happen after a launch that
  // worked); else what slow_check(t0) decided -- it is asked off the fast path, every 4096 spins, and answers kWait to go on.
  template <class Launch, class SlowCheck>
  int await(uint64_t n, Backoff& bo, Launch launch_kernel, SlowCheck slow_check) {
    if (!running && !start(launch_kernel)) {
      withdraw(false);  // nobody will read it
      return 0;
    }
    const double t0 = now_seconds();
    for (unsigned spins = 1;; spins++) {
      if (answered(n)) return 1;
      if (gone()) {
        if (answered(n)) return 1;
        running = false;
        if (!start(launch_kernel)) {
          withdraw(false);
          return 0;
        }
      }
      if ((spins & 0xfff) == 0) {
        const int verdict = slow_check(t0);
        if (verdict != kWait) return verdict;
      }
      bo.pause();
    }
  }

  // a lingering agent is told to go and waited for (finalize; nothing else needs it: it goes by itself)
  void stop() {
    const uint64_t n = ++seq;
    __atomic_store_n((uint64_t*)&cmd[3], n << 32, __ATOMIC_RELEASE);  // (polled by the agent while it is written: atomic, like post's)
    __atomic_store_n((uint64_t*)&cmd[0], 2ull | (n << 24), __ATOMIC_RELEASE);
    Backoff bo;
    const double t0 = now_seconds();
    while (!gone() && now_seconds() - t0 < 5.0) bo.pause();
    running = false;
  }
};

AgentLine recv_line(xmpi_comm* c) { return {c->p2p_cmd, c->agent_seq, c->agent_running, c->agent_stream, c->device}; }
AgentLine ll_line(xmpi_comm* c) { return {c->ll_cmd, c->ll_agent_seq, c->ll_agent_running, c->ll_agent_stream, c->device}; }

}  // namespace

// ---- the receive agent: a copy-and-ack kernel that lingers (sched.hip p2p_agent_kernel) ------------------------------------
// One command at a time per communicator.  Returns true when the agent copied the message and wrote both acks; false: the
// caller launches the ordinary kernel (the agent could not be started).
bool agent_submit(xmpi_comm* c, void* dst, const void* from, size_t bytes, MailEntry* m) {
  if (c->p2p_agent_us <= 0 || !c->p2p_cmd_dev || !c->p2p_rec || !c->ctl_dev || bytes == 0 || bytes > ((size_t)512 << 10)) return false;  // (longer messages: the ordinary kernel's wide grid)
  // One command at a time.  The reference promises concurrent Receives on different {peer, tag} (mpi.go:121-125): a Receive
  // that finds the agent busy with somebody else's message does not queue up behind it -- the launch-per-message kernel on
  // this call's own stream serves it in parallel.
  std::unique_lock<std::mutex> g(c->agent_mu, std::try_to_lock);
  if (!g.owns_lock()) return false;
  AgentLine line = recv_line(c);
  const uint64_t mail_off = (uint64_t)((char*)&m->state - (char*)c->ctl->base());
  const uint64_t seq = line.post((uint64_t)(uintptr_t)from, (uint64_t)(uintptr_t)dst, mail_off & 0xffffffffull, bytes);
  auto launch = [&](hipStream_t s) {
    P2PAgentArgs a;
    memset(&a, 0, sizeof a);
    a.cmd = c->p2p_cmd_dev;
    a.rec = c->p2p_rec;
    a.ctl_dev = (uint64_t)(uintptr_t)c->ctl_dev;
    a.seq0 = seq;
    a.launch = (c->p2p_agent_launch_no + 1) & 0x7fffff;
    a.alone_bytes = 64 << 10;
    a.patience_ticks = (uint64_t)c->p2p_agent_us * 100;  // wall_clock64 runs at 100 MHz
    a.mail_done_value = MAIL_DONE;
    const hipError_t e = launch_p2p_agent(a, 8, s);  // (32 blocks: the 31 that watch a word in device memory slowed block 0 down -- 6.2 us instead of 4.5)
    if (e == hipSuccess) {
      c->p2p_agent_launch_no++;  // numbers the launches (never reset); p2p_agent_launches beside it is the caller's diagnostic count
      c->p2p_agent_launches++;
    }
    return e;
  };
  // Off the fast path, now and then: an agent that faulted (an unmapped payload), a queue that was torn down or a job that
  // was aborted must not leave this thread spinning with the lock held.  The stream is idle only when the agent has ended:
  // if it ended without serving this command and without saying "gone", it is broken -- the ordinary kernel takes over
  // (and reports whatever is wrong with the payload through its own error path).
  auto slow_check = [&](double t0) {
    bool give_up = c->ctl->aborted() || (c->timeout_s > 0 && now_seconds() - t0 > (double)c->timeout_s);
    if (!give_up) {
      const hipError_t e = hipStreamQuery(c->agent_stream);
      (void)hipGetLastError();
      if (e != hipErrorNotReady) give_up = !line.answered(seq) && !line.gone();
    }
    if (!give_up) return kWait;
    if (line.answered(seq)) return 1;
    line.withdraw(true);
    c->agent_running = false;
    return 0;
  };
  Backoff bo;
  if (line.await(seq, bo, launch, slow_check) != 1) return false;
  c->p2p_agent_served++;
  return true;
}

void p2p_agent_stop(xmpi_comm* c) {
  std::lock_guard<std::mutex> g(c->agent_mu);
  if (!c->agent_running || !c->p2p_cmd) return;
  recv_line(c).stop();
}

// ---- the LL agent: a one-block kernel that lingers behind a blocking small collective (ll.hip ll_agent_kernel) -------------
// The caller holds coll_mu (dsync.cpp dsync_ll), so there is one command at a time by construction.  1: the agent ran the
// collective and everything it wrote is visible; 0: not taken (no agent, broken, job aborted) -- nothing has happened that a
// launched LL kernel of the same epoch would not repeat line for line; -1: the agent took it and never answered within the
// no-progress limit (+ 5 s) -- the collective has FAILED (the job's abort flag is set): the caller must not launch anything for this
// epoch beside an agent that may still run.
int agent_submit_ll(xmpi_comm* c, const void* send, void* recv, size_t bytes, int ll_coll, int root, int dtype, int op, bool consecutive) {
  if (c->ll_agent_us <= 0 || !c->ll_cmd_dev || !c->dsync_ok || !c->dpage || c->size < 2 || c->size > kDsyncRanks || bytes == 0 ||
      bytes > kLLMaxPayload)
    return 0;
  // (a reduction of an 8-bit float type is launched: the agent's kernel does not know the two types, and three bits do not name them)
  if (dtype_is_f8(dtype) && (ll_coll == LL_ALLREDUCE || ll_coll == LL_REDUCE)) return 0;
  AgentLine line = ll_line(c);
  if (c->ll_agent_running && line.gone()) c->ll_agent_running = false;  // it said it went: started again below
  static_assert(XMPI_OP_COUNT <= 8, "an LL command names its operator in three bits (kernels.h): a ninth operator needs another layout");
  static_assert(kAgentLLConsecutiveShift - kAgentLLOpShift == 3, "... and these are the three");
  // The dtype has three bits too, and XMPI_F8E4M3 / XMPI_F8E5M2 (7, 8) do not both fit: the field is written for the seven types the
  // agent's folds know and is 0 for the 8-bit floats, which come here for bcast / allgather only (their reductions were declined
  // above) -- copies of bytes, for which the agent never reads the field.  A type the agent is to FOLD needs a place in the field first.
  static_assert(XMPI_BF16 < 8 && kAgentLLOpShift - kAgentLLDtypeShift == 3, "the seven dtypes the agent folds are named in three bits");
  static_assert(XMPI_DTYPE_COUNT == 9, "a new dtype: decline its reductions above, or widen the field");
  const int cmd_dtype = dtype_is_f8(dtype) ? 0 : dtype;
  const uint64_t meta = (uint64_t)(ll_coll & 3) | ((uint64_t)(root & 15) << kAgentLLRootShift) |
                        ((uint64_t)(cmd_dtype & 7) << kAgentLLDtypeShift) | ((uint64_t)(op & 7) << kAgentLLOpShift) |
                        ((uint64_t)(consecutive ? 1 : 0) << kAgentLLConsecutiveShift);
  const uint64_t seq = line.post((uint64_t)(uintptr_t)send, (uint64_t)(uintptr_t)recv, meta, bytes);
  auto launch = [&](hipStream_t s) {
    LLAgentArgs a;
    memset(&a, 0, sizeof a);
    a.cmd = c->ll_cmd_dev;
    a.seq0 = seq;
    a.patience_ticks = (uint64_t)c->ll_agent_us * 100;  // wall_clock64 runs at 100 MHz
    for (int p = 0; p < c->size; p++) a.ll.page[p] = c->peer_page[p];
    a.ll.me = c->rank;
    a.ll.n = c->size;
    a.ll.epoch_floor = c->dsync_base;
    a.ll.host_epoch = c->dsync_status_dev ? (uint64_t*)(c->dsync_status_dev + 2) : nullptr;
    a.ll.abort_word = c->dsync_abort_dev;
    a.ll.status = c->dsync_status_dev;
    a.ll.spin_limit = spin_limit_ticks(c);
    const hipError_t e = launch_ll_agent(a, s);
    if (e == hipSuccess) c->ll_agent_launches++;
    return e;
  };
  Backoff bo;
  bo.idle = [](void* p) { dsync_service((xmpi_comm*)p); };  // (a peer may be waiting for this rank to map a buffer before it can start)
  bo.idle_arg = c;
  // Off the fast path, now and then: an agent that faulted, a queue that was torn down -- the stream is idle only when the
  // agent has ended; if it ended without serving this command and without saying "gone", it is broken and the launched kernel
  // takes over.  A dead PEER is the agent's own business (ll_gather gives up within the no-progress limit and says why);
  // this thread allows it that limit and a little more.
  auto slow_check = [&](double t0) {
    const hipError_t e = hipStreamQuery(c->ll_agent_stream);
    (void)hipGetLastError();
    if (e != hipErrorNotReady && !line.answered(seq) && !line.gone()) {
      // the stream is idle: the agent has ENDED, without serving this command and without saying "gone" -- broken.  Nothing of it
      // runs any more, so the launched kernel may take the epoch over.
      c->ll_agent_running = false;
      line.withdraw(true);  // (the number stays consumed: a relaunch starts at the next one)
      return 0;
    }
    if (c->timeout_s > 0 && now_seconds() - t0 > (double)c->timeout_s + 5.0) {
      if (line.answered(seq)) return 1;
      // The agent may still be INSIDE the collective (its own clock should have cut its waits short by now): a second kernel for
      // the same epoch beside it would store into the same slots and answer the same record.  The collective has failed: the
      // job's abort flag makes the agent's waits end, and nothing reuses the record before it has gone or its stream is idle.
      c->ctl->set_abort(XMPI_ERR_TIMEOUT);
      line.withdraw(true);
      const double t1 = now_seconds();
      while (!line.gone() && hipStreamQuery(c->ll_agent_stream) == hipErrorNotReady && now_seconds() - t1 < 10.0) bo.pause();
      (void)hipGetLastError();
      c->ll_agent_running = false;
      return -1;
    }
    return kWait;
  };
  return line.await(seq, bo, launch, slow_check);
}

void ll_agent_stop(xmpi_comm* c) {
  if (!c->ll_agent_running || !c->ll_cmd) return;
  ll_line(c).stop();
}

}  // namespace xmpi
