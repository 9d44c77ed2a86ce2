// engine.cpp -- executes a step table (plan.h) over the HBM pipes.  Compiled by hipcc as host code.
// (The blocking tagged Send / Receive: p2p.cpp; the host side of the lingering agents: agent.cpp.)
//
// Data path of one SEND/RECV pair (replaces gob-encode -> net.Conn -> gob-decode of
// network.go:518-625):
//   sender    : peer copy  local HBM -> slot in the RECEIVER's window (xGMI write, SDMA or copy
//               kernel) on send_stream[peer]; when its event completes the host publishes
//               head++ in the shared control block.
//   receiver  : sees head > consumed, launches the reduction / copy-out kernel on
//               recv_stream[peer] reading the slot from its own HBM; when that completes it
//               publishes tail++ (the ack of network.go:616-624, one counter instead of a message).
// Nothing on the GPU ever blocks on another process: a step is enqueued only once its
// cross-process precondition already holds, so streams cannot deadlock however HIP maps them
// to hardware queues.  Same-process dependencies are chained with events (no host round trip).
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

hipEvent_t ev_get(xmpi_comm* c, bool timed) {
  std::lock_guard<std::mutex> g(c->ev_mu);
  std::vector<hipEvent_t>& pool = timed ? c->ev_timed_free : c->ev_free;
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, timed ? hipEventDefault : hipEventDisableTiming) != hipSuccess) return nullptr;
  return e;
}

void ev_put(xmpi_comm* c, hipEvent_t e, bool timed) {
  std::lock_guard<std::mutex> g(c->ev_mu);
  if (e) (timed ? c->ev_timed_free : c->ev_free).push_back(e);
}

bool is_device_pointer(const void* p) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // unregistered host memory: clear the sticky error
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeArray;
}

namespace {

// Ranks hosted by threads of one process enqueue onto one stream: serialise each step's enqueue so a
// profiled launch is bracketed by ITS events only.
std::mutex g_shared_stream_mu;
struct SharedStreamLock {
  std::unique_lock<std::mutex> l;
  explicit SharedStreamLock(const xmpi_comm* c) {
    if (c->shared_stream) l = std::unique_lock<std::mutex>(g_shared_stream_mu);
  }
};

struct InFlight {
  int step;
  hipEvent_t done;         // completion tracking (not needed for stream-ordered steps)
  hipEvent_t start, stop;  // only for profiled launches: attached to the dispatch itself
  int prof_kind;
  size_t prof_bytes;
  std::vector<int> more;   // further steps completed by the same launch (batched copies)
};

int peer_copy(xmpi_comm* c, void* dst, const void* src, size_t bytes, hipStream_t s, hipEvent_t es, hipEvent_t ee) {
  if (c->copy_engine == 1) {
    XMPI_HIP(launch_copy(dst, src, bytes, s, es, ee));
  } else {
    if (es) XMPI_HIP(hipEventRecord(es, s));
    XMPI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    if (ee) XMPI_HIP(hipEventRecord(ee, s));
  }
  return XMPI_OK;
}

struct Exec {
  xmpi_comm* c;
  const Plan& plan;
  char* bufs[3];
  int dtype, op;
  int N, L;
  size_t es;

  std::vector<std::deque<int>> sq, rq;  // per (peer, lane): pending SEND / RECV steps in FIFO order
  std::deque<int> lq;                   // LOCAL_COPY / REDUCE_N
  std::vector<uint8_t> state;           // 0 pending, 1 issued, 2 complete
  std::vector<hipEvent_t> ev;
  std::vector<int> stream_of;
  std::vector<char*> slot_ptr;          // RECV_*: the slot this step reads
  std::vector<uint64_t> slot_seq;
  std::vector<uint64_t> out_seq;        // fused steps: sequence number of the slot they push
  std::vector<std::deque<InFlight>> fl;  // per stream, completion is in issue order
  std::vector<std::deque<char>> unreleased;  // per (peer, lane): popped slots not yet released
  std::vector<std::deque<char>> unpublished;  // per (peer, lane): pushed slots whose head is not yet out
  size_t remaining;
  double last_progress;
  bool eager_used = false;
  std::vector<InFlight> prof_pending;  // sampled eager steps: timed after the final sync

  Exec(xmpi_comm* comm, const Plan& p, const void* sb, void* rb, int dt, int o)
      : c(comm), plan(p), dtype(dt), op(o), N(comm->size), L(comm->lanes) {
    bufs[BUF_SEND] = (char*)const_cast<void*>(sb);
    bufs[BUF_RECV] = (char*)rb;
    bufs[BUF_TEMP] = (char*)comm->temp;
    es = xmpi_dtype_size((xmpi_dtype)dt);
    const size_t n = p.steps.size();
    sq.resize((size_t)N * L);
    rq.resize((size_t)N * L);
    state.assign(n, 0);
    ev.assign(n, nullptr);
    stream_of.assign(n, -1);
    slot_ptr.assign(n, nullptr);
    slot_seq.assign(n, 0);
    out_seq.assign(n, 0);
    fl.resize((size_t)2 * N + 3);
    unreleased.resize((size_t)N * L);
    unpublished.resize((size_t)N * L);
    remaining = n;
    for (size_t i = 0; i < n; i++) {
      const Step& s = p.steps[i];
      if (s.kind == STEP_SEND) sq[(size_t)s.peer * L + s.lane].push_back((int)i);
      else if (s.kind == STEP_RECV_REDUCE || s.kind == STEP_RECV_COPY || s.kind == STEP_RECV_HOLD)
        rq[(size_t)s.peer * L + s.lane].push_back((int)i);
      else if (is_fused(s)) {  // pops one pipe and pushes another: in FIFO order on both
        rq[(size_t)s.peer * L + s.lane].push_back((int)i);
        sq[(size_t)s.peer2 * L + s.lane2].push_back((int)i);
      } else lq.push_back((int)i);
    }
    last_progress = now_seconds();
  }

  static bool is_fused(const Step& s) { return s.kind == STEP_RECV_REDUCE_SEND || s.kind == STEP_RECV_COPY_SEND; }

  hipStream_t stream(int sid) const {
    if (sid < N) return c->send_stream[sid];
    if (sid < 2 * N) return c->recv_stream[sid - N];
    if (sid == 2 * N + 1) return c->batch_send_stream;
    if (sid == 2 * N + 2) return c->batch_recv_stream;
    return c->local_stream;
  }

  // a step may be enqueued once its dependencies are enqueued (chained with hipStreamWaitEvent)
  bool deps_issued(const Step& s) const {
    for (int d = 0; d < s.ndeps; d++)
      if (state[(size_t)s.deps[d]] < 1) return false;
    return true;
  }

  int chain_deps(const Step& s, int sid) {
    for (int d = 0; d < s.ndeps; d++) {
      const int j = s.deps[d];
      if (state[(size_t)j] == 1 && stream(stream_of[(size_t)j]) != stream(sid) && ev[(size_t)j])
        XMPI_HIP(hipStreamWaitEvent(stream(sid), ev[(size_t)j], 0));
    }
    return XMPI_OK;
  }

  int begin_op(int i, InFlight* f, int prof_kind, size_t prof_bytes) {
    f->step = i;
    f->done = f->start = f->stop = nullptr;
    f->prof_kind = prof_kind;
    f->prof_bytes = prof_bytes;
    if (c->prof_on && prof_kind >= 0 &&
        (c->prof_seq[prof_kind]++ % (uint64_t)std::max<long>(1, c->prof_every)) == 0) {
      f->start = ev_get(c, true);
      f->stop = ev_get(c, true);
      if (!f->start || !f->stop) return XMPI_ERR_HIP;
    }
    return XMPI_OK;
  }

  // eager = the consumer of this step's effect runs on the SAME in-order stream (ranks hosted by
  // one process on one GPU): stream order already guarantees what the completion event would, so
  // the counters are published at enqueue time and no event is recorded at all.
  int end_op(int i, int sid, InFlight* f, bool eager) {
    stream_of[(size_t)i] = sid;
    for (int j : f->more) stream_of[(size_t)j] = sid;
    if (eager) {
      if (f->start) prof_pending.push_back(*f);
      eager_used = true;
      state[(size_t)i] = 2;
      remaining--;
      publish(plan.steps[(size_t)i], i);
      for (int j : f->more) {
        state[(size_t)j] = 2;
        remaining--;
        publish(plan.steps[(size_t)j], j);
      }
      return XMPI_OK;
    }
    f->done = ev_get(c, false);
    if (!f->done) return XMPI_ERR_HIP;
    XMPI_HIP(hipEventRecord(f->done, stream(sid)));
    ev[(size_t)i] = f->done;
    state[(size_t)i] = 1;
    for (int j : f->more) {
      ev[(size_t)j] = f->done;
      state[(size_t)j] = 1;
    }
    fl[(size_t)sid].push_back(*f);
    return XMPI_OK;
  }

  bool coloc(int peer) const { return c->shared_stream && c->peer_coloc[peer]; }

  void release_slot(int peer, int lane, uint64_t seq) {
    std::deque<char>& u = unreleased[(size_t)peer * L + lane];
    uint64_t& base = c->recvd_released[peer][lane];
    u[(size_t)(seq - base)] = 1;
    while (!u.empty() && u.front()) {
      u.pop_front();
      base++;
    }
    c->ctl->pipe(peer, c->rank, lane)->tail.v.store(base, std::memory_order_release);
  }

  int account(const InFlight& f) {
    if (f.start) {
      float ms = 0.f;
      XMPI_HIP(hipEventElapsedTime(&ms, f.start, f.stop));
      ProfCounter& pc = c->prof[f.prof_kind];
      pc.add(ms, f.prof_bytes);
      ev_put(c, f.start, true);
      ev_put(c, f.stop, true);
    }
    if (f.done) ev_put(c, f.done, false);
    return XMPI_OK;
  }

  // pushes of one pipe may complete out of order (batched and single launches run on different
  // streams): head only advances over a gap-free prefix of filled slots
  void publish_push(int peer, int lane, uint64_t seq) {
    std::deque<char>& u = unpublished[(size_t)peer * L + lane];
    uint64_t& base = c->sent_done[peer][lane];
    u[(size_t)(seq - base)] = 1;
    while (!u.empty() && u.front()) {
      u.pop_front();
      base++;
    }
    c->ctl->pipe(c->rank, peer, lane)->head.v.store(base, std::memory_order_release);
  }

  // make the effect of a finished (or stream-ordered) step visible to the peer
  void publish(const Step& s, int step) {
    switch (s.kind) {
      case STEP_SEND:
        publish_push(s.peer, s.lane, slot_seq[(size_t)step]);
        break;
      case STEP_RECV_REDUCE:
      case STEP_RECV_COPY:
        release_slot(s.peer, s.lane, slot_seq[(size_t)step]);
        break;
      case STEP_RECV_REDUCE_SEND:
      case STEP_RECV_COPY_SEND:
        publish_push(s.peer2, s.lane2, out_seq[(size_t)step]);
        release_slot(s.peer, s.lane, slot_seq[(size_t)step]);
        break;
      case STEP_REDUCE_N:
        for (int k = 0; k < s.nsrcs; k++)
          if (s.srcs[k] >= 0) {
            const Step& h = plan.steps[(size_t)s.srcs[k]];
            release_slot(h.peer, h.lane, slot_seq[(size_t)s.srcs[k]]);
          }
        break;
      default:
        break;
    }
  }

  int complete(const InFlight& f) {
    int rc = account(f);
    if (rc) return rc;
    ev[(size_t)f.step] = nullptr;
    state[(size_t)f.step] = 2;
    remaining--;
    publish(plan.steps[(size_t)f.step], f.step);
    for (int j : f.more) {
      ev[(size_t)j] = nullptr;
      state[(size_t)j] = 2;
      remaining--;
      publish(plan.steps[(size_t)j], j);
    }
    return XMPI_OK;
  }

  // ---- batched launches: everything of one kind that is ready right now goes out in ONE launch ------
  enum BatchKind { BATCH_SEND = 0, BATCH_RECV_COPY, BATCH_RECV_REDUCE, BATCH_RRS, BATCH_RCS, BATCH_KINDS };

  static int kind_of_batch(int bk) {
    switch (bk) {
      case BATCH_SEND: return STEP_SEND;
      case BATCH_RECV_COPY: return STEP_RECV_COPY;
      case BATCH_RECV_REDUCE: return STEP_RECV_REDUCE;
      case BATCH_RRS: return STEP_RECV_REDUCE_SEND;
      default: return STEP_RECV_COPY_SEND;
    }
  }

  bool can_pop(const Step& s) const {
    return c->ctl->pipe(s.peer, c->rank, s.lane)->head.v.load(std::memory_order_acquire) > c->recvd[s.peer][s.lane];
  }
  bool can_push(int peer, int lane) const {
    const uint64_t tail = c->ctl->pipe(c->rank, peer, lane)->tail.v.load(std::memory_order_acquire);
    return c->sent[peer][lane] - tail < (uint64_t)c->fifo_depth;
  }

  // is step i (the front of a queue) of batch kind bk and ready to be launched right now?
  bool batch_ready(int i, int bk) const {
    const Step& s = plan.steps[(size_t)i];
    if (s.kind != kind_of_batch(bk) || !deps_issued(s) || s.bytes > c->slot_bytes) return false;
    switch (bk) {
      case BATCH_SEND: return can_push(s.peer, s.lane);
      case BATCH_RECV_COPY:
      case BATCH_RECV_REDUCE: return can_pop(s);
      default: {  // fused: next in line on BOTH of its pipes, data in, room out
        const std::deque<int>& in = rq[(size_t)s.peer * L + s.lane];
        const std::deque<int>& out = sq[(size_t)s.peer2 * L + s.lane2];
        return !in.empty() && in.front() == i && !out.empty() && out.front() == i && can_pop(s) &&
               can_push(s.peer2, s.lane2);
      }
    }
  }

  int issue_batch(const std::vector<int>& steps, int bk) {
    void *dst[kMaxBatch], *dst2[kMaxBatch];
    const void *src[kMaxBatch], *opa[kMaxBatch];
    size_t bytes[kMaxBatch], counts[kMaxBatch];
    const int n = (int)steps.size();
    const int sid = bk == BATCH_SEND ? 2 * N + 1 : 2 * N + 2;
    size_t total = 0, written = 0;
    bool eager = c->shared_stream;
    for (int k = 0; k < n; k++) {
      const int i = steps[(size_t)k];
      const Step& s = plan.steps[(size_t)i];
      int rc = chain_deps(s, sid);
      if (rc) return rc;
      dst[k] = dst2[k] = nullptr;
      src[k] = opa[k] = nullptr;
      if (bk != BATCH_SEND) {  // pop the incoming slot
        const uint64_t seq = c->recvd[s.peer][s.lane];
        char* slot = c->window + c->coll_slot_off(s.peer, s.lane, seq);
        slot_ptr[(size_t)i] = slot;
        slot_seq[(size_t)i] = seq;
        c->recvd[s.peer][s.lane] = seq + 1;
        unreleased[(size_t)s.peer * L + s.lane].push_back(0);
        src[k] = slot;
        opa[k] = bufs[s.src_buf] + s.src_off;  // reductions: the local operand
        if (bk != BATCH_RRS || s.keep_local) dst[k] = bufs[s.dst_buf] + s.dst_off;
        if (!coloc(s.peer)) eager = false;
      }
      if (bk == BATCH_SEND || bk == BATCH_RRS || bk == BATCH_RCS) {  // claim the outgoing slot
        const int peer = bk == BATCH_SEND ? s.peer : s.peer2, lane = bk == BATCH_SEND ? s.lane : s.lane2;
        const uint64_t seq = c->sent[peer][lane];
        char* remote = c->peer_window[peer] + c->coll_slot_off(c->rank, lane, seq);
        c->sent[peer][lane] = seq + 1;
        unpublished[(size_t)peer * L + lane].push_back(0);
        if (bk == BATCH_SEND) {
          slot_seq[(size_t)i] = seq;
          dst[k] = remote;
          src[k] = bufs[s.src_buf] + s.src_off;
        } else {
          out_seq[(size_t)i] = seq;
          dst2[k] = remote;
        }
        if (!coloc(peer)) eager = false;
      }
      bytes[k] = s.bytes;
      counts[k] = s.bytes / es;
      total += s.bytes;
      written += s.bytes * (size_t)((dst[k] ? 1 : 0) + (dst2[k] ? 1 : 0));
    }
    InFlight f;
    SharedStreamLock lk(c);
    const bool reduce = bk == BATCH_RECV_REDUCE || bk == BATCH_RRS;
    const int pk = bk == BATCH_SEND ? PROF_PEER : (reduce ? PROF_REDUCE2 : PROF_COPY);
    const size_t pb = bk == BATCH_SEND ? total : (reduce ? 2 * total + written : total + written);
    int rc = begin_op(steps[0], &f, pk, pb);
    if (rc) return rc;
    for (int k = 1; k < n; k++) f.more.push_back(steps[(size_t)k]);
    if (reduce)
      XMPI_HIP(launch_reduce2_batch(dst, dst2, opa, src, counts, n, dtype, op, stream(sid), f.start, f.stop));
    else
      XMPI_HIP(launch_copy_batch(dst, dst2, src, bytes, n, stream(sid), f.start, f.stop));
    return end_op(steps[0], sid, &f, eager);
  }

  // Returns the number of steps issued, <0 on error.  Plain sends and slot drains batch only when
  // they are kernels (copy_engine 1) and at least two are ready; the fused ring steps exist only as
  // kernels and always go through here, alone if need be.
  int try_batches() {
    int issued = 0;
    for (int bk = 0; bk < BATCH_KINDS; bk++) {
      const bool fused = bk == BATCH_RRS || bk == BATCH_RCS;
      if (!fused && !c->batch_copies) continue;
      if ((bk == BATCH_SEND || bk == BATCH_RECV_COPY) && c->copy_engine != 1) continue;
      std::vector<std::deque<int>>& qs = bk == BATCH_SEND ? sq : rq;
      const size_t max_group = c->batch_copies ? (size_t)kMaxBatch : 1;
      for (;;) {
        std::vector<int> ready;
        for (auto& q : qs) {
          if (q.empty() || ready.size() >= max_group) continue;
          if (batch_ready(q.front(), bk)) ready.push_back(q.front());
        }
        if (ready.size() < (fused ? 1u : 2u)) break;  // a single plain step takes the ordinary path
        int rc = issue_batch(ready, bk);
        if (rc) return rc;
        for (int i : ready) {
          const Step& s = plan.steps[(size_t)i];
          if (bk == BATCH_SEND) sq[(size_t)s.peer * L + s.lane].pop_front();
          else rq[(size_t)s.peer * L + s.lane].pop_front();
          if (fused) sq[(size_t)s.peer2 * L + s.lane2].pop_front();
        }
        issued += (int)ready.size();
      }
    }
    return issued;
  }

  // returns 1 if issued, 0 if not ready, <0 on error
  int try_send(int i) {
    const Step& s = plan.steps[(size_t)i];
    if (is_fused(s) || !deps_issued(s)) return 0;  // fused steps are launched by try_batches
    const uint64_t seq = c->sent[s.peer][s.lane];
    const uint64_t tail = c->ctl->pipe(c->rank, s.peer, s.lane)->tail.v.load(std::memory_order_acquire);
    if (seq - tail >= (uint64_t)c->fifo_depth) return 0;
    if (s.bytes > c->slot_bytes) return XMPI_ERR_ARG;
    const int sid = s.peer;
    int rc = chain_deps(s, sid);
    if (rc) return rc;
    InFlight f;
    SharedStreamLock lk(c);  // [start marker, launch, done marker] stay contiguous on a shared stream
    rc = begin_op(i, &f, PROF_PEER, s.bytes);
    if (rc) return rc;
    char* dst = c->peer_window[s.peer] + c->coll_slot_off(c->rank, s.lane, seq);
    rc = peer_copy(c, dst, bufs[s.src_buf] + s.src_off, s.bytes, stream(sid), f.start, f.stop);
    if (rc) return rc;
    c->sent[s.peer][s.lane] = seq + 1;
    slot_seq[(size_t)i] = seq;
    unpublished[(size_t)s.peer * L + s.lane].push_back(0);
    rc = end_op(i, sid, &f, coloc(s.peer));
    if (rc) return rc;
    return 1;
  }

  int try_recv(int i) {
    const Step& s = plan.steps[(size_t)i];
    if (is_fused(s) || !deps_issued(s)) return 0;  // fused steps are launched by try_batches
    const uint64_t seq = c->recvd[s.peer][s.lane];
    const uint64_t head = c->ctl->pipe(s.peer, c->rank, s.lane)->head.v.load(std::memory_order_acquire);
    if (head <= seq) return 0;
    char* slot = c->window + c->coll_slot_off(s.peer, s.lane, seq);
    slot_ptr[(size_t)i] = slot;
    slot_seq[(size_t)i] = seq;
    c->recvd[s.peer][s.lane] = seq + 1;
    unreleased[(size_t)s.peer * L + s.lane].push_back(0);
    if (s.kind == STEP_RECV_HOLD) {
      state[(size_t)i] = 2;
      remaining--;
      return 1;
    }
    const int sid = N + s.peer;
    int rc = chain_deps(s, sid);
    if (rc) return rc;
    InFlight f;
    SharedStreamLock lk(c);  // [start marker, launch, done marker] stay contiguous on a shared stream
    if (s.kind == STEP_RECV_REDUCE) {
      rc = begin_op(i, &f, PROF_REDUCE2, 3 * s.bytes);
      if (rc) return rc;
      XMPI_HIP(launch_reduce2(bufs[s.dst_buf] + s.dst_off, bufs[s.src_buf] + s.src_off, slot, s.bytes / es, dtype,
                              op, stream(sid), f.start, f.stop));
    } else {
      rc = begin_op(i, &f, PROF_COPY, 2 * s.bytes);
      if (rc) return rc;
      XMPI_HIP(launch_copy(bufs[s.dst_buf] + s.dst_off, slot, s.bytes, stream(sid), f.start, f.stop));
    }
    return end_op(i, sid, &f, coloc(s.peer)) ? XMPI_ERR_HIP : 1;
  }

  int try_local(int i) {
    const Step& s = plan.steps[(size_t)i];
    if (!deps_issued(s)) return 0;
    const int sid = 2 * N;
    if (s.kind == STEP_REDUCE_N) {
      for (int k = 0; k < s.nsrcs; k++)
        if (s.srcs[k] >= 0 && state[(size_t)s.srcs[k]] == 0) return 0;
    }
    int rc = chain_deps(s, sid);
    if (rc) return rc;
    InFlight f;
    SharedStreamLock lk(c);  // [start marker, launch, done marker] stay contiguous on a shared stream
    if (s.kind == STEP_REDUCE_N) {
      const void* srcs[kMaxSrcs];
      for (int k = 0; k < s.nsrcs; k++)
        srcs[k] = (s.srcs[k] < 0) ? (const void*)(bufs[s.src_buf] + s.src_off) : (const void*)slot_ptr[(size_t)s.srcs[k]];
      rc = begin_op(i, &f, PROF_REDUCEN, (size_t)(s.nsrcs + 1) * s.bytes);
      if (rc) return rc;
      XMPI_HIP(launch_reduce_n(bufs[s.dst_buf] + s.dst_off, srcs, s.nsrcs, s.bytes / es, dtype, op, stream(sid),
                               f.start, f.stop));
    } else {
      rc = begin_op(i, &f, PROF_COPY, 2 * s.bytes);
      if (rc) return rc;
      const char* src = bufs[s.src_buf] + s.src_off;
      char* dst = bufs[s.dst_buf] + s.dst_off;
      XMPI_HIP(launch_copy(dst, src, s.bytes, stream(sid), f.start, f.stop));
    }
    bool eager = c->shared_stream;
    if (s.kind == STEP_REDUCE_N)
      for (int k = 0; k < s.nsrcs; k++)
        if (s.srcs[k] >= 0 && !coloc(plan.steps[(size_t)s.srcs[k]].peer)) eager = false;
    return end_op(i, sid, &f, eager) ? XMPI_ERR_HIP : 1;
  }

  int run() {
    Backoff bo;
    arm(bo, c);
    while (remaining > 0) {
      bool progressed = false;
      {
        const int nb = try_batches();
        if (nb < 0) return nb;
        progressed = nb > 0;
      }
      for (auto& q : sq)
        while (!q.empty()) {
          int r = try_send(q.front());
          if (r < 0) return r;
          if (r == 0) break;
          q.pop_front();
          progressed = true;
        }
      for (auto& q : rq)
        while (!q.empty()) {
          int r = try_recv(q.front());
          if (r < 0) return r;
          if (r == 0) break;
          q.pop_front();
          progressed = true;
        }
      // local steps may become ready out of order (different pieces wait on different pipes)
      for (size_t k = 0; k < lq.size();) {
        int r = try_local(lq[k]);
        if (r < 0) return r;
        if (r == 1) {
          lq.erase(lq.begin() + (long)k);
          progressed = true;
        } else {
          k++;
          if (k >= 8) break;  // look a few steps ahead only
        }
      }
      for (auto& q : fl)
        while (!q.empty()) {
          hipError_t e = hipEventQuery(q.front().done);
          if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            break;
          }
          if (e != hipSuccess) return hip_fail(e, "hipEventQuery", __FILE__, __LINE__);
          int rc = complete(q.front());
          if (rc) return rc;
          q.pop_front();
          progressed = true;
        }
      if (progressed) {
        last_progress = now_seconds();
        bo.n = 0;
        continue;
      }
      if (c->ctl->aborted()) {
        set_last_error(c->ctl->abort_reason());
        return XMPI_ERR_PEER;
      }
      if (c->timeout_s > 0 && now_seconds() - last_progress > (double)c->timeout_s) {
        set_last_error("collective made no progress for " + std::to_string(c->timeout_s) + " s");
        return XMPI_ERR_TIMEOUT;
      }
      bo.pause();
    }
    if (eager_used) {  // the call is blocking: this rank's stream-ordered work must have finished
      hipEvent_t fin = ev_get(c, false);
      if (!fin) return XMPI_ERR_HIP;
      XMPI_HIP(hipEventRecord(fin, c->local_stream));
      const double ts = now_seconds();
      XMPI_HIP(hipEventSynchronize(fin));
      c->last_sync_us = (now_seconds() - ts) * 1e6;
      ev_put(c, fin, false);
      for (const InFlight& f : prof_pending) {
        int rc = account(f);
        if (rc) return rc;
      }
      prof_pending.clear();
    }
    return XMPI_OK;
  }
};

}  // namespace

int run_plan(xmpi_comm* c, const Plan& plan, const void* sendbuf, void* recvbuf, int dtype, int op) {
  if (plan.steps.empty()) return XMPI_OK;
  if (!c->windows_ok) {  // (api.cpp collective() sends every call of such a job to the device-synchronised path: not reached)
    set_last_error("the staged step tables need the HBM windows, which this job could not map (xmpi_degraded)");
    return XMPI_ERR_UNSUPPORTED;
  }
  RoctxRange range("xmpi:run_plan steps=%zu", plan.steps.size());
  {
    const int src = ensure_streams(c);
    if (src != XMPI_OK) return src;
  }
  if (plan.temp_bytes > c->temp_bytes) {
    if (c->temp) XMPI_HIP(hipFree(c->temp));
    c->temp = nullptr;
    c->temp_bytes = 0;
    XMPI_HIP(hipMalloc(&c->temp, plan.temp_bytes));
    c->temp_bytes = plan.temp_bytes;
  }
  const double t0 = now_seconds();
  Exec ex(c, plan, sendbuf, recvbuf, dtype, op);
  c->last_sync_us = 0;
  int rc = ex.run();
  c->last_run_us = (now_seconds() - t0) * 1e6;
  if (rc != XMPI_OK) {
    c->ctl->set_abort(rc);
    // leave no work behind that still references pooled events
    (void)hipDeviceSynchronize();
  }
  return rc;
}

}  // namespace xmpi
