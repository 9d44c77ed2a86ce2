// p2p.cpp -- the blocking tagged Send / Receive (the reference's whole API: mpi.go Send / Receive, network.go:518-625), probe
// and the deferred wait of xmpi_send_nowait.  Compiled by hipcc as host code.
//
// A message is a MAIL ENTRY of the ordered pair (sender -> receiver) in the shared control block (ctl.h MailEntry):
//   FREE -> CLAIMED (sender: claim_entry) -> POSTED (header filled) -> MATCHED (receiver: match_entry) -> DONE (the receiver's
//   verdict: `finish`, or the copy kernel / the receive agent on its behalf) -> FREE (sender: await_ack -> release_entry).
// A sender that finds nobody takes a POSTED entry back (`withdraw`).  How the payload travels is one function each:
//   sender    send_through_host_lane | (stand_in_without_windows ->) offer -> push_through_slots
//   receiver  recv_from_host_lane | recv_direct_to_host | recv_direct_to_device | recv_through_slots
// Nothing on the GPU ever blocks on another process: every copy is enqueued only once its cross-process precondition holds.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

namespace {

hipStream_t p2p_stream_get(xmpi_comm* c) {
  std::lock_guard<std::mutex> g(c->p2p_mu);
  if (!c->p2p_streams.empty()) {
    hipStream_t s = c->p2p_streams.back();
    c->p2p_streams.pop_back();
    return s;
  }
  return stream_acquire(c->device);
}

void p2p_stream_put(xmpi_comm* c, hipStream_t s) {
  std::lock_guard<std::mutex> g(c->p2p_mu);
  c->p2p_streams.push_back(s);
}

struct TagGuard {
  xmpi_comm* c;
  std::set<std::pair<int, int>>* reg;
  std::pair<int, int> key;
  bool held = false;
  TagGuard(xmpi_comm* comm, std::set<std::pair<int, int>>* r, int peer, int tag) : c(comm), reg(r), key(peer, tag) {
    std::lock_guard<std::mutex> g(c->p2p_mu);
    held = reg->insert(key).second;
  }
  ~TagGuard() {
    if (held) {
      std::lock_guard<std::mutex> g(c->p2p_mu);
      reg->erase(key);
    }
  }
};

struct StreamLease {
  xmpi_comm* c;
  hipStream_t s;
  explicit StreamLease(xmpi_comm* comm) : c(comm), s(p2p_stream_get(comm)) {}
  ~StreamLease() {
    if (s) p2p_stream_put(c, s);
  }
};

bool timed_out(xmpi_comm* c, double t0) { return c->timeout_s > 0 && now_seconds() - t0 > (double)c->timeout_s; }

// ---- the mail entry's operations, once each --------------------------------------------------------------------------------

// an entry goes back to its pair: by the sender, after the verdict, a withdrawal, or a claim that was never posted
void release_entry(MailEntry* m) {
  m->pipe.head.v.store(0, std::memory_order_relaxed);
  m->pipe.tail.v.store(0, std::memory_order_relaxed);
  m->state.store(MAIL_FREE, std::memory_order_release);
}

// A send that found no matching receive within XMPI_TIMEOUT_S takes its message back: the entry goes from POSTED to
// FREE and the call returns XMPI_ERR_TIMEOUT with the job intact (the reference would block for ever,
// network.go:569; a test harness prefers an error).  false = a receive matched it in the meantime: keep waiting.
bool withdraw(MailEntry* m) {
  uint32_t expect = MAIL_POSTED;
  if (!m->state.compare_exchange_strong(expect, MAIL_CLAIMED, std::memory_order_acq_rel)) return false;
  release_entry(m);
  return true;
}

// the receiver's verdict -- the ack of network.go:616-624: the only host-side writer of MAIL_DONE
void finish(MailEntry* m, int status) {
  m->status.store(status, std::memory_order_release);
  m->state.store(MAIL_DONE, std::memory_order_release);
}

// One side of a message and its waiting: the clock restarts with every sign of progress.
struct Side {
  xmpi_comm* c;
  int peer, tag;
  hipStream_t s;  // the call's leased stream
  MailEntry* m = nullptr;
  int entry = -1;
  Backoff bo;
  double tp;
  Side(xmpi_comm* comm, int p, int t, hipStream_t stream) : c(comm), peer(p), tag(t), s(stream), tp(now_seconds()) { arm(bo, c); }
  void progressed() {
    tp = now_seconds();
    bo.n = 0;
  }
};

struct Sender : Side {
  using Side::Side;
  // One turn of a sender's wait.  XMPI_OK: look again.  XMPI_ERR_PEER: the job was aborted.  XMPI_ERR_TIMEOUT: nothing moved for
  // XMPI_TIMEOUT_S and the message could be taken back -- nothing is in flight (may_withdraw), no receive has matched it: the entry
  // is free again, the error text is set, the job goes on.
  int step(bool may_withdraw = true) {
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (c->timeout_s > 0 && now_seconds() - tp > (double)c->timeout_s) {
      if (may_withdraw && withdraw(m)) {
        set_last_error("send to rank " + std::to_string(peer) + " tag " + std::to_string(tag) + ": no matching receive");
        return XMPI_ERR_TIMEOUT;
      }
      tp = now_seconds();  // matched a moment ago: the receiver is copying
    }
    bo.pause();
    return XMPI_OK;
  }
  // how a transport leaves with an error: after a withdrawal (above) the job is intact; after anything else -- a peer failed,
  // a HIP call failed -- the entry is in an unknown state and the job cannot continue
  int fail(int rc) {
    if (rc != XMPI_ERR_TIMEOUT) c->ctl->set_abort(rc);
    return rc;
  }
};

struct Receiver : Side {
  using Side::Side;
  // one turn of a matched receiver's wait for the sender's next piece
  int step() {
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (c->timeout_s > 0 && now_seconds() - tp > (double)c->timeout_s) {
      set_last_error("receive: sender stalled");
      return XMPI_ERR_TIMEOUT;
    }
    bo.pause();
    return XMPI_OK;
  }
  int fail(int rc) {
    c->ctl->set_abort(rc);
    return rc;
  }
};

// sender: FREE -> CLAIMED, a mail entry of the ordered pair (me -> dest)
int claim_entry(Sender& tx) {
  xmpi_comm* c = tx.c;
  const double t0 = now_seconds();
  for (;;) {
    for (int e = 0; e < kMailEntries; e++) {
      MailEntry* cand = c->ctl->mail(c->rank, tx.peer, e);
      uint32_t expect = MAIL_FREE;
      if (cand->state.compare_exchange_strong(expect, MAIL_CLAIMED, std::memory_order_acq_rel)) {
        tx.m = cand;
        tx.entry = e;
        return XMPI_OK;
      }
    }
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (timed_out(c, t0)) {
      set_last_error("send: no free mail entry towards rank " + std::to_string(tx.peer));
      return XMPI_ERR_TIMEOUT;
    }
    tx.bo.pause();
  }
}

// receiver: POSTED -> MATCHED, the entry of (src -> me) that carries the tag
int match_entry(Receiver& rx) {
  xmpi_comm* c = rx.c;
  const double t0 = now_seconds();
  for (;;) {
    for (int e = 0; e < kMailEntries; e++) {
      MailEntry* cand = c->ctl->mail(rx.peer, c->rank, e);
      if (cand->state.load(std::memory_order_acquire) == MAIL_POSTED && cand->tag == rx.tag) {
        uint32_t expect = MAIL_POSTED;
        if (cand->state.compare_exchange_strong(expect, MAIL_MATCHED, std::memory_order_acq_rel)) {
          if (cand->tag != rx.tag) {  // withdrawn and re-posted with another tag between the look and the claim
            cand->state.store(MAIL_POSTED, std::memory_order_release);
            continue;
          }
          rx.m = cand;
          rx.entry = e;
          return XMPI_OK;
        }
      }
    }
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (timed_out(c, t0)) {
      set_last_error("receive from rank " + std::to_string(rx.peer) + " tag " + std::to_string(rx.tag) + ": no matching send");
      return XMPI_ERR_TIMEOUT;
    }
    rx.bo.pause();
  }
}

// rendezvous: wait for the receiver's verdict (network.go:569 waits for the ack message), free the entry
int await_ack(xmpi_comm* c, MailEntry* m, int dest, int tag) {
  Sender tx(c, dest, tag, nullptr);
  tx.m = m;
  while (m->state.load(std::memory_order_acquire) != MAIL_DONE) {
    const int rc = tx.step();
    if (rc != XMPI_OK) return tx.fail(rc);
  }
  const int rc = m->status.load(std::memory_order_acquire);
  release_entry(m);
  return rc;
}

// The tail of every Send.  wait_ack = false (xmpi_send_nowait): the payload has left the caller's buffer -- it sits in the
// receiver's window or in the host lane --, the entry is parked and {dest, tag} stays reserved until p2p_wait.
int leave_pending_or_await(Sender& tx, TagGuard& tg, bool wait_ack) {
  if (!wait_ack) {
    std::lock_guard<std::mutex> g(tx.c->p2p_mu);
    tx.c->pending_sends[{tx.peer, tx.tag}] = tx.m;
    tg.held = false;
    return XMPI_OK;
  }
  return await_ack(tx.c, tx.m, tx.peer, tx.tag);
}

// ---- the piece pipeline: copies on one stream, an event behind each, retired in order ----------------------------------------
struct PiecePipe {
  xmpi_comm* c;
  hipStream_t s;
  std::deque<hipEvent_t> inflight;

  // e: what enqueuing the piece's copy on `s` returned; a pooled event is recorded behind it
  int issue(hipError_t e, const char* what) {
    hipEvent_t ev = (e == hipSuccess) ? ev_get(c, false) : nullptr;
    if (e == hipSuccess && ev) e = hipEventRecord(ev, s);
    if (e != hipSuccess || !ev) return hip_fail(e, what, __FILE__, __LINE__);
    inflight.push_back(ev);
    return XMPI_OK;
  }
  // takes off every piece that has completed, in order: on_done() publishes the new count (the sender's head, the receiver's tail)
  template <class F>
  int retire(F on_done, bool* progressed) {
    while (!inflight.empty()) {
      hipError_t e = hipEventQuery(inflight.front());
      if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        break;
      }
      if (e != hipSuccess) return hip_fail(e, "hipEventQuery", __FILE__, __LINE__);
      ev_put(c, inflight.front(), false);
      inflight.pop_front();
      on_done();
      *progressed = true;
    }
    return XMPI_OK;
  }
  // on every exit: nothing in flight may outlive the call, the events go back to the pool
  void drain() {
    if (inflight.empty()) return;
    (void)hipStreamSynchronize(s);
    while (!inflight.empty()) {
      ev_put(c, inflight.front(), false);
      inflight.pop_front();
    }
  }
};

hipError_t device_copy(xmpi_comm* c, void* dst, const void* src, size_t n, hipStream_t s) {
  return c->copy_engine == 1 ? launch_copy(dst, src, n, s) : hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, s);
}

// The arguments of one pull kernel (sched.hip p2p_pull_kernel) and its completion word: the kernel's last block writes *id into
// *done_word, which the calling thread polls.  The mail_* fields stay null: the caller that wants the kernel to write the ack sets them.
P2PPullArgs pull_args(xmpi_comm* c, void* dst, const void* src, size_t bytes, uint64_t* id, volatile uint64_t** done_word) {
  *id = c->p2p_pull_next.fetch_add(1, std::memory_order_relaxed) + 1;
  const int slot = (int)(*id % (uint64_t)xmpi_comm::kP2PDoneSlots);
  *done_word = c->p2p_done + 4 * (xmpi_comm::kP2PDoneSlots + slot);
  P2PPullArgs pa;
  memset(&pa, 0, sizeof pa);
  pa.dst = dst;
  pa.src = src;
  pa.bytes = bytes;
  pa.ticket = c->p2p_tickets + slot;
  pa.host_done = c->p2p_done_dev + 4 * (xmpi_comm::kP2PDoneSlots + slot);
  pa.done_value = *id;
  return pa;
}

// Blocks of the pull kernel (sched.hip p2p_pull_kernel: 16 KiB in flight per block; every block acquires before and releases
// after its share -- a cache operation each).  What bounds a message is the memory it comes out of.  Sender and receiver on ONE
// GPU: the sender's HBM, but the per-block cache operations cost more than extra blocks bring -- 16 MiB, half round trip, r04:
// 32 blocks 28.9 us, 64 23.6, 128 25.2, 256 34.0, 512 50.8, 1024 92.2 (1 MiB: 11.0 with 32, 12.2 with 64 and more) -- so one
// block per 256 KiB, at least 16, at most 512.  Different GPUs: ONE link; blocks beyond bandwidth x latency in flight add
// nothing but contention, so the cap follows the rate xmpi_link_probe measured for this pair (link_gbps; the nominal 64 GB/s
// per direction until it has run) at ~4 us of round trip, with a margin of 2.  "p2p_grid_cap" / XMPI_P2P_GRID_CAP override.
long p2p_pull_cap(const xmpi_comm* c, int peer, size_t bytes) {
  if (c->p2p_grid_cap > 0) return c->p2p_grid_cap;
  const RankInfo* a = c->ctl->info(c->rank);
  const RankInfo* b = c->ctl->info(peer);
  if (strncmp(a->busid, b->busid, sizeof a->busid) == 0) return std::max<long>(16, std::min<long>((long)(bytes >> 18), 512));
  const double gbps = c->link_gbps[peer] > 0 ? c->link_gbps[peer] : 64.0;
  const long blocks = (long)(2.0 * gbps * 1e9 * 4e-6 / 16384.0) + 1;
  return std::max<long>(16, std::min<long>(blocks, 256));
}

constexpr size_t kP2PBounceBytes = (size_t)256 << 10;  // device -> host slice through pinned memory up to this length

// ---- the sender's transports ---------------------------------------------------------------------------------------------------

// A payload in HOST memory -- what the reference's callers pass: Go slices (network.go:518, bounce.go:96) -- travels
// through the entry's host lane in the shared segment: the first pieces are in place before the message is posted, the
// rest follows as the receiver drains.  (Staging it through both GPUs' HBM took 3 PCIe crossings, a hipMalloc and two
// events per message: 40 us one way for 8 bytes -- the reference's loopback TCP takes 8.)
// Assumes: the entry is CLAIMED, its header filled; posts it (DIRECT_HOST).  The receiver writes the ack (recv_from_host_lane).
int send_through_host_lane(Sender& tx, const void* buf, size_t bytes) {
  xmpi_comm* c = tx.c;
  MailEntry* m = tx.m;
  const size_t piece = c->ctl->host_lane_bytes() / kHostLaneSlots;
  const uint64_t np = (bytes + piece - 1) / piece;
  char* lane = c->ctl->host_lane(c->rank, tx.peer, tx.entry);
  uint64_t filled = 0;
  auto fill = [&]() {
    const size_t off = (size_t)filled * piece;
    memcpy(lane + (size_t)(filled % kHostLaneSlots) * piece, (const char*)buf + off, std::min(piece, bytes - off));
    filled++;
  };
  while (filled < np && filled < (uint64_t)kHostLaneSlots) fill();
  m->pipe.head.v.store(filled, std::memory_order_relaxed);
  m->direct.store(DIRECT_HOST, std::memory_order_relaxed);
  m->state.store(MAIL_POSTED, std::memory_order_release);
  tx.progressed();
  while (filled < np) {
    if (filled - m->pipe.tail.v.load(std::memory_order_acquire) < (uint64_t)kHostLaneSlots) {
      fill();
      m->pipe.head.v.store(filled, std::memory_order_release);
      tx.progressed();
      continue;
    }
    if (m->state.load(std::memory_order_acquire) == MAIL_DONE) break;  // the receiver gave up (truncate ...)
    const int rc = tx.step();
    if (rc != XMPI_OK) return tx.fail(rc);
  }
  return XMPI_OK;
}

struct StandIn {
  void* p = nullptr;
  ~StandIn() {
    if (p) (void)heap_free(p);
  }
};

// A job that voted its windows away (xmpi_init: a rank could not map one) has no mail slots: a payload the receiver cannot
// pull as it lies -- unregistered device memory, a host slice with the host lanes off -- first goes into a registered block of
// this rank (one local copy), and THAT is offered.  xmpi_send_nowait needs the slots: not in this mode.
// Assumes: the entry is CLAIMED and not posted; on an error it goes back.  The caller keeps `standin` until after the ack.
int stand_in_without_windows(Sender& tx, const void* buf, size_t bytes, bool dev_src, bool wait_ack, StandIn* standin) {
  xmpi_comm* c = tx.c;
  BufRef probe;
  if (!wait_ack) {
    release_entry(tx.m);
    set_last_error("send_nowait: this job runs without windows (xmpi_degraded): no mail slots to leave the payload in");
    return XMPI_ERR_UNSUPPORTED;
  }
  if (dev_src && zc_export(c, buf, bytes, &probe)) return XMPI_OK;  // (registered: offered as it lies)
  standin->p = heap_alloc(c->device, bytes);
  if (!standin->p || hipMemcpyAsync(standin->p, buf, bytes, hipMemcpyDefault, tx.s) != hipSuccess || hipStreamSynchronize(tx.s) != hipSuccess) {
    (void)hipGetLastError();
    release_entry(tx.m);
    set_last_error("send: no registered block for the payload (this job runs without windows)");
    return XMPI_ERR_NOMEM;
  }
  return XMPI_OK;
}

// A registered source (xmpi_malloc / xmpi_register) is offered to the receiver, which then copies
// straight out of it: one pass over the data and one xGMI crossing instead of slot-in + slot-out.
// (A job without windows has no mail slots: the offer is the ONLY way a device payload travels there, whatever p2p_direct_bytes
// says -- "always through the mail slots" (< 0) or a threshold above this message would leave the receiver waiting for slots
// nobody fills, for ever by default.)
// Assumes: the entry is CLAIMED, its header filled; posts it (DIRECT_OFFERED or DIRECT_NONE) and, if offered, waits for the
// matching receive to decide.  *push: the payload is still to be pushed through the slots.  An accepted offer is copied and
// acknowledged by the receiver.
int offer(Sender& tx, const void* buf, size_t bytes, bool dev_now, bool wait_ack, bool* push) {
  xmpi_comm* c = tx.c;
  MailEntry* m = tx.m;
  const bool must_offer = !c->windows_ok && bytes > 0;
  const bool offered = wait_ack && dev_now && (must_offer || (c->p2p_direct_bytes >= 0 && bytes >= (size_t)std::max<long>(1, c->p2p_direct_bytes))) &&
                       zc_export(c, buf, bytes, &m->src);
  m->direct.store(offered ? DIRECT_OFFERED : DIRECT_NONE, std::memory_order_relaxed);
  m->state.store(MAIL_POSTED, std::memory_order_release);
  tx.progressed();
  if (offered) {  // rendezvous first: the matching receive decides how the payload travels
    while (m->direct.load(std::memory_order_acquire) == DIRECT_OFFERED && m->state.load(std::memory_order_acquire) != MAIL_DONE) {
      const int rc = tx.step();
      if (rc != XMPI_OK) return tx.fail(rc);  // (a withdrawal: nothing was pushed, the entry is free again, the job goes on)
    }
  }
  *push = m->direct.load(std::memory_order_acquire) != DIRECT_ACCEPTED && m->state.load(std::memory_order_acquire) != MAIL_DONE &&
          (c->windows_ok || bytes == 0);
  // (no windows: a receiver that could not take the offer has answered with its error -- MAIL_DONE -- and nothing is pushed)
  return XMPI_OK;
}

// The payload goes piece by piece into the slots of this entry in the RECEIVER's window (a host payload: bounced through this
// rank's HBM), at most p2p_depth pieces ahead of the receiver's tail; head is published as each copy completes.
// Assumes: the entry is POSTED or MATCHED.  The receiver writes the ack (recv_through_slots).
int push_through_slots(Sender& tx, const void* buf, size_t bytes, bool dev_src) {
  xmpi_comm* c = tx.c;
  MailEntry* m = tx.m;
  const size_t slot = c->p2p_slot_bytes;
  const uint64_t npieces = (bytes + slot - 1) / slot;
  const uint64_t depth = (uint64_t)c->p2p_depth;
  PiecePipe pipe{c, tx.s, {}};
  uint64_t issued = 0, published = 0;
  int rc = XMPI_OK;
  void* stage = nullptr;
  if (!dev_src && npieces > 0) {  // host payload: bounce through this rank's HBM
    if (hipMalloc(&stage, std::min<size_t>(bytes, depth * slot)) != hipSuccess)
      rc = hip_fail(hipGetLastError(), "hipMalloc(stage)", __FILE__, __LINE__);
  }
  tx.progressed();
  while (rc == XMPI_OK && published < npieces) {
    bool progressed = false;
    if (issued < npieces && issued - m->pipe.tail.v.load(std::memory_order_acquire) < depth) {
      const size_t off = (size_t)issued * slot, n = std::min(slot, bytes - off);
      char* dst = c->peer_window[tx.peer] + c->p2p_slot_off(c->rank, tx.entry, issued);
      hipError_t e;
      if (dev_src) {
        e = device_copy(c, dst, (const char*)buf + off, n, tx.s);
      } else {
        char* st = (char*)stage + (size_t)(issued % depth) * slot;
        e = hipMemcpyAsync(st, (const char*)buf + off, n, hipMemcpyHostToDevice, tx.s);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, st, n, hipMemcpyDeviceToDevice, tx.s);
      }
      rc = pipe.issue(e, "p2p send copy");
      if (rc != XMPI_OK) break;
      issued++;
      progressed = true;
    }
    rc = pipe.retire([&] { m->pipe.head.v.store(++published, std::memory_order_release); }, &progressed);
    if (rc != XMPI_OK) break;
    if (progressed) {
      tx.progressed();
      continue;
    }
    if (m->state.load(std::memory_order_acquire) == MAIL_DONE) break;  // receiver gave up (truncate...)
    rc = tx.step(pipe.inflight.empty());  // (the slots are full and nobody drains them: take the message back)
  }
  pipe.drain();
  if (stage) (void)hipFree(stage);
  return rc == XMPI_OK ? XMPI_OK : tx.fail(rc);
}

}  // namespace

// wait_ack = false is the reference author's intended Send (commented out at mpi.go:132-152): return
// once the payload has left the caller's buffer; p2p_wait() later collects the receiver's confirmation
// and frees the {dest, tag} pair.
int p2p_send(xmpi_comm* c, const void* buf, size_t bytes, int dtype, int dest, int tag, bool wait_ack) {
  // {dest,tag} unique among concurrent sends (mpi.go:121-125; the reference panics at
  // network.go:469, here it is an error code the Go shim turns into mpi.TagExists)
  RoctxRange range("xmpi:send dest=%d tag=%d bytes=%zu", dest, tag, bytes);
  TagGuard tg(c, &c->send_tags, dest, tag);
  if (!tg.held) {
    set_last_error("tag " + std::to_string(tag) + " already in use sending to " + std::to_string(dest));
    return XMPI_ERR_TAG_EXISTS;
  }
  StreamLease lease(c);
  if (!lease.s) return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
  const bool dev_src = bytes == 0 || heap_owns(buf) || is_device_pointer(buf);  // (the arena lookup is the cheap answer)
  Sender tx(c, dest, tag, lease.s);
  int rc = claim_entry(tx);
  if (rc != XMPI_OK) return rc;
  tx.m->tag = tag;
  tx.m->dtype = dtype;
  tx.m->bytes = bytes;
  tx.m->status.store(XMPI_OK, std::memory_order_relaxed);
  StandIn standin;  // (a job without windows: freed on every exit, after the ack)
  if (!dev_src && bytes > 0 && c->ctl->host_lane_bytes() > 0) {
    rc = send_through_host_lane(tx, buf, bytes);
  } else {
    if (!c->windows_ok && bytes > 0) {
      rc = stand_in_without_windows(tx, buf, bytes, dev_src, wait_ack, &standin);
      if (rc != XMPI_OK) return rc;
      if (standin.p) buf = standin.p;
    }
    bool push = false;
    rc = offer(tx, buf, bytes, dev_src || standin.p, wait_ack, &push);
    if (rc == XMPI_OK && push) rc = push_through_slots(tx, buf, bytes, dev_src);
  }
  if (rc != XMPI_OK) return rc;
  return leave_pending_or_await(tx, tg, wait_ack);
}

int p2p_wait(xmpi_comm* c, int dest, int tag) {
  MailEntry* m = nullptr;
  {
    std::lock_guard<std::mutex> g(c->p2p_mu);
    auto it = c->pending_sends.find({dest, tag});
    if (it == c->pending_sends.end()) {
      set_last_error("wait: no send to rank " + std::to_string(dest) + " with tag " + std::to_string(tag) + " is outstanding");
      return XMPI_ERR_ARG;
    }
    m = it->second;
    c->pending_sends.erase(it);
  }
  const int rc = await_ack(c, m, dest, tag);
  std::lock_guard<std::mutex> g(c->p2p_mu);
  c->send_tags.erase({dest, tag});
  return rc;
}

// Wait for a message {src, tag} to be posted and report its size without consuming it (lets a
// host-language binding size the destination the way gob's in-place decode does, network.go:597).
int p2p_probe(xmpi_comm* c, int src, int tag, size_t* bytes, int* dtype) {
  const double t0 = now_seconds();
  Backoff bo;
  arm(bo, c);
  for (;;) {
    for (int e = 0; e < kMailEntries; e++) {
      MailEntry* m = c->ctl->mail(src, c->rank, e);
      if (m->state.load(std::memory_order_acquire) == MAIL_POSTED && m->tag == tag) {
        if (bytes) *bytes = m->bytes;
        if (dtype) *dtype = m->dtype;
        return XMPI_OK;
      }
    }
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (timed_out(c, t0)) {
      set_last_error("probe from rank " + std::to_string(src) + " tag " + std::to_string(tag) + ": no matching send");
      return XMPI_ERR_TIMEOUT;
    }
    bo.pause();
  }
}

namespace {

// ---- the receiver's transports: each assumes the entry is MATCHED and the verdict on dtype and length was "fits" --------------

// The payload comes through the entry's host lane (send_through_host_lane): a host destination takes it with memcpy, piece by
// piece; a device destination by a kernel out of the (registered) lane, as many pieces at a time as have arrived.
// Who writes the ack: the receive agent when it took the message, else this function.
int recv_from_host_lane(Receiver& rx, void* buf, size_t bytes, bool dev_dst) {
  xmpi_comm* c = rx.c;
  MailEntry* m = rx.m;
  const size_t piece = c->ctl->host_lane_bytes() / kHostLaneSlots;
  const uint64_t np = (bytes + piece - 1) / piece;
  const char* lane = c->ctl->host_lane(rx.peer, c->rank, rx.entry);
  uint64_t taken = 0;
  int rc = XMPI_OK;
  rx.progressed();
  if (dev_dst && c->lanes_dev_ok && c->p2p_kernel_ack && np <= (uint64_t)kHostLaneSlots) {
    // a message that fits the ring lies there in one piece (it was complete before it was posted): the receive agent pulls it
    // out of the pinned lane like it pulls a message out of a peer's HBM, and writes the ack -- no DMA call, no event
    while (rc == XMPI_OK && m->pipe.head.v.load(std::memory_order_acquire) < np) rc = rx.step();
    if (rc == XMPI_OK && agent_submit(c, buf, c->ctl_dev + (lane - (const char*)c->ctl->base()), bytes, m)) {
      __atomic_fetch_add(&c->p2p_lane_count, 1, __ATOMIC_RELAXED);
      return XMPI_OK;
    }
  }
  // Longer messages stream through the ring.  A host destination takes the pieces with memcpy.  A device destination has a
  // kernel pull every run of pieces that has arrived (the GPU reads the pinned lane itself; its last block writes a completion
  // word this thread polls) -- one DMA call + event per 64 KiB piece took twice as long (r03 session 14: 1 MiB 357 us per round
  // trip instead of 240), and so does the runtime's staged copy when the lane could not be pinned (the fallback below).
  const bool pull = dev_dst && c->lanes_dev_ok && c->p2p_kernel_ack && c->p2p_done_dev && c->p2p_tickets;
  uint64_t pending = 0, pending_id = 0;
  volatile uint64_t* pending_word = nullptr;
  while (rc == XMPI_OK && taken < np) {
    bool progressed = false;
    const uint64_t head = m->pipe.head.v.load(std::memory_order_acquire);
    if (head > taken && !dev_dst) {
      for (uint64_t k = taken; k < head; k++) {
        const size_t off = (size_t)k * piece;
        memcpy((char*)buf + off, lane + (size_t)(k % kHostLaneSlots) * piece, std::min(piece, bytes - off));
      }
      taken = head;
      m->pipe.tail.v.store(taken, std::memory_order_release);
      progressed = true;
    } else if (head > taken && pull && !pending) {
      const uint64_t first = taken % kHostLaneSlots, run = std::min<uint64_t>(head - taken, kHostLaneSlots - first);  // contiguous in the lane
      const size_t off = (size_t)taken * piece;
      const auto pa = pull_args(c, (char*)buf + off, c->ctl_dev + ((lane + (size_t)first * piece) - (const char*)c->ctl->base()),
                                std::min((size_t)run * piece, bytes - off), &pending_id, &pending_word);
      const long gx = std::max<long>(1, std::min<long>(16, (long)((pa.bytes + 16383) >> 14)));
      if (launch_p2p_pull(pa, (int)gx, rx.s) != hipSuccess) {
        rc = hip_fail(hipGetLastError(), "p2p pull out of the host lane", __FILE__, __LINE__);
        break;
      }
      pending = run;
      progressed = true;
    } else if (head > taken && dev_dst && !pull) {
      for (uint64_t k = taken; k < head && rc == XMPI_OK; k++) {
        const size_t off = (size_t)k * piece;
        if (hipMemcpyAsync((char*)buf + off, lane + (size_t)(k % kHostLaneSlots) * piece, std::min(piece, bytes - off), hipMemcpyHostToDevice,
                           rx.s) != hipSuccess)
          rc = hip_fail(hipGetLastError(), "p2p receive from the host lane", __FILE__, __LINE__);
      }
      if (rc == XMPI_OK && hipStreamSynchronize(rx.s) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipStreamSynchronize", __FILE__, __LINE__);
      taken = head;
      m->pipe.tail.v.store(taken, std::memory_order_release);
      progressed = true;
    }
    if (pending && __atomic_load_n((const uint64_t*)pending_word, __ATOMIC_ACQUIRE) == pending_id) {
      taken += pending;
      pending = 0;
      m->pipe.tail.v.store(taken, std::memory_order_release);
      progressed = true;
    }
    if (progressed) {
      rx.progressed();
      continue;
    }
    rc = rx.step();
  }
  if (pending) (void)hipStreamSynchronize(rx.s);  // (an error above: the kernel in flight must not outlive the call)
  if (rc != XMPI_OK) return rx.fail(rc);
  __atomic_fetch_add(&c->p2p_lane_count, 1, __ATOMIC_RELAXED);
  finish(m, XMPI_OK);
  return XMPI_OK;
}

// The sender's buffer is registered and mapped here (`from`): one copy device -> HOST memory (the caller handed a slice), no slots
// in between.  Assumes DIRECT_ACCEPTED is stored.  Who writes the ack: the receive agent when it took the message, else this function.
int recv_direct_to_host(Receiver& rx, void* buf, const void* from, size_t bytes) {
  xmpi_comm* c = rx.c;
  if (c->p2p_kernel_ack && bytes <= kP2PBounceBytes) {
    // short: the receive agent copies into a pinned block and acks; the slice gets it with memcpy (the runtime's copy into
    // pageable memory is a staged, synchronous affair of 20 us)
    std::lock_guard<std::mutex> g(c->p2p_bounce_mu);
    if (!c->p2p_bounce) {
      void* p = nullptr;
      void* dev = nullptr;
      if (hipHostMalloc(&p, kP2PBounceBytes, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dev, p, 0) == hipSuccess) {
        c->p2p_bounce = (char*)p;
        c->p2p_bounce_dev = (char*)dev;
      } else {
        (void)hipGetLastError();
        if (p) (void)hipHostFree(p);
      }
    }
    if (c->p2p_bounce_dev && agent_submit(c, c->p2p_bounce_dev, from, bytes, rx.m)) {
      memcpy(buf, c->p2p_bounce, bytes);
      __atomic_fetch_add(&c->p2p_direct_count, 1, __ATOMIC_RELAXED);
      return XMPI_OK;
    }
  }
  if (hipMemcpyAsync(buf, from, bytes, hipMemcpyDeviceToHost, rx.s) != hipSuccess || hipStreamSynchronize(rx.s) != hipSuccess)
    return rx.fail(hip_fail(hipGetLastError(), "p2p direct copy to the host", __FILE__, __LINE__));
  __atomic_fetch_add(&c->p2p_direct_count, 1, __ATOMIC_RELAXED);
  finish(rx.m, XMPI_OK);
  return XMPI_OK;
}

// The sender's buffer is registered and mapped here (`from`): copy straight out of it into device memory (mapped once per
// allocation).  Assumes DIRECT_ACCEPTED is stored.  Who copies and who writes the ack, in this order: the lingering receive
// agent (both); one pull kernel (both); a plain copy on the leased stream, then this function.
int recv_direct_to_device(Receiver& rx, void* buf, const void* from, size_t bytes) {
  xmpi_comm* c = rx.c;
  MailEntry* m = rx.m;
  int rc = XMPI_OK;
  if (c->p2p_kernel_ack && agent_submit(c, buf, from, bytes, m)) {  // the lingering agent took it: no launch at all
    __atomic_fetch_add(&c->p2p_direct_count, 1, __ATOMIC_RELAXED);
    return XMPI_OK;
  }
  if (c->p2p_kernel_ack && c->ctl_dev && c->p2p_done_dev && c->p2p_tickets) {
    // ONE kernel copies and acks: its last block writes DONE into the message's mail entry (the sender's host thread
    // polls it: the ack of network.go:616-624, without this rank's host in between) and the completion word this
    // thread polls.  Nothing in it waits for anybody.
    uint64_t id = 0;
    volatile uint64_t* done = nullptr;
    auto pa = pull_args(c, buf, from, bytes, &id, &done);
    char* mdev = c->ctl_dev + ((char*)m - (char*)c->ctl->base());
    pa.mail_state = (uint32_t*)(mdev + ((char*)&m->state - (char*)m));
    pa.mail_status = (int32_t*)(mdev + ((char*)&m->status - (char*)m));
    pa.mail_done_value = MAIL_DONE;
    long gx = (long)((bytes + 16383) >> 14);  // a 16 KiB tile per block and pass; how many blocks: p2p_pull_cap
    gx = std::max<long>(1, std::min<long>(gx, p2p_pull_cap(c, rx.peer, bytes)));
    hipError_t e = launch_p2p_pull(pa, (int)gx, rx.s);
    if (e != hipSuccess) rc = hip_fail(e, "p2p pull kernel", __FILE__, __LINE__);
    rx.bo.n = 0;
    while (rc == XMPI_OK && __atomic_load_n((const uint64_t*)done, __ATOMIC_ACQUIRE) != id) {
      if ((rx.bo.n & 1023u) == 1023u && c->ctl->aborted()) rc = XMPI_ERR_PEER;
      rx.bo.pause();
    }
    if (rc != XMPI_OK) return rx.fail(rc);
    __atomic_fetch_add(&c->p2p_direct_count, 1, __ATOMIC_RELAXED);
    return XMPI_OK;
  }
  PiecePipe pipe{c, rx.s, {}};  // (the whole message as one piece)
  rc = pipe.issue(device_copy(c, buf, from, bytes, rx.s), "p2p direct copy");
  rx.bo.n = 0;
  while (rc == XMPI_OK && !pipe.inflight.empty()) {
    bool progressed = false;
    rc = pipe.retire([] {}, &progressed);
    if (rc != XMPI_OK || progressed) continue;
    if (c->ctl->aborted()) rc = XMPI_ERR_PEER;
    rx.bo.pause();
  }
  pipe.drain();
  if (rc != XMPI_OK) return rx.fail(rc);
  __atomic_fetch_add(&c->p2p_direct_count, 1, __ATOMIC_RELAXED);
  finish(m, XMPI_OK);
  return XMPI_OK;
}

// a message this job has no way to carry: both sides get the error, the job goes on
int refuse_without_windows(MailEntry* m, const char* why) {
  set_last_error(why);
  finish(m, XMPI_ERR_UNSUPPORTED);
  return XMPI_ERR_UNSUPPORTED;
}

// The payload arrives piece by piece in this entry's slots of this rank's window (push_through_slots); every piece is copied
// out as its head is published, tail follows as each copy completes.  This function writes the ack.
int recv_through_slots(Receiver& rx, void* buf, size_t bytes, bool dev_dst) {
  xmpi_comm* c = rx.c;
  MailEntry* m = rx.m;
  __atomic_fetch_add(&c->p2p_staged_count, 1, __ATOMIC_RELAXED);
  const size_t slot = c->p2p_slot_bytes;
  const uint64_t npieces = (bytes + slot - 1) / slot;
  PiecePipe pipe{c, rx.s, {}};
  uint64_t issued = 0, drained = 0;
  int rc = XMPI_OK;
  rx.progressed();
  while (rc == XMPI_OK && drained < npieces) {
    bool progressed = false;
    if (issued < npieces && m->pipe.head.v.load(std::memory_order_acquire) > issued) {
      const size_t off = (size_t)issued * slot, n = std::min(slot, bytes - off);
      const char* from = c->window + c->p2p_slot_off(rx.peer, rx.entry, issued);
      rc = pipe.issue(dev_dst ? device_copy(c, (char*)buf + off, from, n, rx.s) : hipMemcpyAsync((char*)buf + off, from, n, hipMemcpyDeviceToHost, rx.s),
                      "p2p recv copy");
      if (rc != XMPI_OK) break;
      issued++;
      progressed = true;
    }
    rc = pipe.retire([&] { m->pipe.tail.v.store(++drained, std::memory_order_release); }, &progressed);
    if (rc != XMPI_OK) break;
    if (progressed) {
      rx.progressed();
      continue;
    }
    rc = rx.step();
  }
  pipe.drain();
  if (rc != XMPI_OK) return rx.fail(rc);
  finish(m, XMPI_OK);
  return XMPI_OK;
}

}  // namespace

int p2p_recv(xmpi_comm* c, void* buf, size_t cap_bytes, int dtype, int src, int tag, size_t* got_bytes) {
  RoctxRange range("xmpi:recv src=%d tag=%d capacity=%zu", src, tag, cap_bytes);
  TagGuard tg(c, &c->recv_tags, src, tag);
  if (!tg.held) {
    set_last_error("tag " + std::to_string(tag) + " already in use receiving from " + std::to_string(src));
    return XMPI_ERR_TAG_EXISTS;
  }
  StreamLease lease(c);
  if (!lease.s) return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
  Receiver rx(c, src, tag, lease.s);
  const int rc = match_entry(rx);
  if (rc != XMPI_OK) return rc;
  MailEntry* m = rx.m;
  const size_t bytes = m->bytes;
  if (got_bytes) *got_bytes = bytes;
  int verdict = XMPI_OK;
  if (m->dtype != dtype) {
    set_last_error("receive: dtype differs from the sender's");
    verdict = XMPI_ERR_ARG;
  } else if (bytes > cap_bytes) {
    set_last_error("receive: message of " + std::to_string(bytes) + " bytes does not fit " + std::to_string(cap_bytes));
    verdict = XMPI_ERR_TRUNCATE;
  }
  if (verdict != XMPI_OK) {
    finish(m, verdict);
    return verdict;
  }
  const bool dev_dst = bytes == 0 || heap_owns(buf) || is_device_pointer(buf);
  const auto how = m->direct.load(std::memory_order_acquire);
  if (how == DIRECT_HOST) return recv_from_host_lane(rx, buf, bytes, dev_dst);
  if (how == DIRECT_OFFERED) {
    void* from = nullptr;
    if (zc_import(c, src, m->src, &from)) {
      m->direct.store(DIRECT_ACCEPTED, std::memory_order_release);
      return dev_dst ? recv_direct_to_device(rx, buf, from, bytes) : recv_direct_to_host(rx, buf, from, bytes);
    }
    if (!c->windows_ok && bytes > 0)  // ... which this job does not have: both sides get the error, the job goes on
      return refuse_without_windows(m, "receive: the sender's buffer cannot be mapped here and this job runs without windows (xmpi_degraded)");
    m->direct.store(DIRECT_DECLINED, std::memory_order_release);  // host destination / not mappable: use the slots
  }
  if (!c->windows_ok && bytes > 0)  // a message that was not even offered (a sender of another mind): there are no slots to wait on
    return refuse_without_windows(m, "receive: the message was posted for the mail slots, which this job does not have (xmpi_degraded)");
  return recv_through_slots(rx, buf, bytes, dev_dst);
}

}  // namespace xmpi
