// dsync_call.cpp -- the lifecycle of a device-synchronised call: what it publishes to the peers and waits to be acknowledged, the
// blocks it borrows and how they go back, the pinned memory host slices pass through, how a blocking call waits, how one rank's
// kernels are kept one at a time across streams -- and DsyncCall, which holds all of that for one call.  HIP calls, waits and
// counters; what is launched is decided elsewhere (dsync_plan.cpp) and launched by the collectives (dsync.cpp, vcoll.cpp,
// dsync_p2p.cpp).
//
// Every wait here serves the peers meanwhile (comm.h arm, which serves only when dsync_ok is set): that flag is set by construction,
// since every entry into these files lies behind dsync_usable (dsync_takes, xmpi_tune, the self-check, xmpi_alltoallv's v_on_device) or
// behind the stream-ordered Send / Receive's own test of it (api.cpp p2p_on_stream_ok).
#include <algorithm>
#include <cstring>

#include "dsync.h"

namespace xmpi {

// the slot of my translation-table row that holds registration `gen`; publishes it if need be.
// *pub_index = how many published entries a peer must have processed to know it.
int dsync_publish(xmpi_comm* c, const BufRef& ref, int* slot_out, uint64_t* pub_index, bool capturing) {
  for (int s = 0; s < kDsyncArenas; s++)
    if (c->dsync_slot_gen[s] == ref.gen) {
      c->dsync_slot_used[s] = c->dsync_epoch + 1;
      *slot_out = s;
      *pub_index = c->dsync_slot_pub[s];
      return XMPI_OK;
    }
  int slot = -1;
  for (int s = 0; s < kDsyncArenas && slot < 0; s++)
    if (c->dsync_slot_gen[s] == 0) slot = s;
  if (slot < 0)  // slots of registrations that have been freed / deregistered since are free again
    for (int s = 0; s < kDsyncArenas; s++)
      if (!registry_alive(c->dsync_slot_gen[s])) {
        c->dsync_slot_gen[s] = 0;
        if (slot < 0) slot = s;
      }
  if (slot < 0) {
    // all slots hold live registrations: re-use the one that has not been used for longest.  Collectives in
    // flight may still name it -- let them finish first (this is rare: > 32 registered allocations in use).
    if (capturing) {  // a synchronisation is not allowed while a stream of the thread captures
      set_last_error("graph capture: the buffer's registration has no translation slot yet (use it in one collective before capturing)");
      return XMPI_ERR_ARG;
    }
    XMPI_HIP(hipDeviceSynchronize());
    slot = 0;
    for (int s = 1; s < kDsyncArenas; s++)
      if (c->dsync_slot_used[s] < c->dsync_slot_used[slot]) slot = s;
  }
  PubTable* pt = c->ctl->published(c->rank);
  const uint64_t n = pt->count.load(std::memory_order_relaxed);
  // the ring must not overwrite an entry a peer has not read yet
  Backoff bo;
  arm(bo, c);
  const double t0 = now_seconds();
  for (;;) {
    uint64_t lo = n;
    for (int p = 0; p < c->size; p++)
      if (p != c->rank) lo = std::min(lo, c->ctl->acked(p, c->rank)->load(std::memory_order_acquire));
    if (n - lo < (uint64_t)kPubRing) break;
    if (c->ctl->aborted()) return XMPI_ERR_PEER;
    if (now_seconds() - t0 > wait_limit(c)) return XMPI_ERR_TIMEOUT;
    dsync_service(c);
    bo.pause();
  }
  PubEntry& e = pt->e[n % kPubRing];
  e.gen = ref.gen;
  e.base = ref.base;
  e.bytes = ref.bytes;
  e.reserved = (uint64_t)slot;
  memcpy(e.handle, ref.handle, sizeof e.handle);
  pt->count.store(n + 1, std::memory_order_release);
  c->dsync_slot_gen[slot] = ref.gen;
  c->dsync_slot_pub[slot] = n + 1;
  c->dsync_slot_used[slot] = c->dsync_epoch + 1;
  *slot_out = slot;
  *pub_index = n + 1;
  return XMPI_OK;
}

int dsync_await_acks(xmpi_comm* c, uint64_t pub_index) {
  Backoff bo;
  arm(bo, c);
  const double t0 = now_seconds();
  for (;;) {
    bool all = true;
    for (int p = 0; p < c->size && all; p++)
      if (p != c->rank && c->ctl->acked(p, c->rank)->load(std::memory_order_acquire) < pub_index) all = false;
    if (all) return XMPI_OK;
    if (c->ctl->aborted()) {
      set_last_error(c->ctl->abort_reason());
      return XMPI_ERR_PEER;
    }
    if (now_seconds() - t0 > wait_limit(c)) {
      set_last_error("a peer did not map a newly registered buffer (is it inside the library at all?)");
      return XMPI_ERR_TIMEOUT;
    }
    dsync_service(c);
    bo.pause();
  }
}

// buffers lent to collectives on a stream (bounce copies of unregistered memory): given back once the
// stream has passed them
static void reap_deferred(xmpi_comm* c, bool wait) {
  for (size_t i = 0; i < c->dsync_deferred.size();) {
    auto& b = c->dsync_deferred[i];
    hipError_t e = wait ? hipEventSynchronize(b.done) : hipEventQuery(b.done);
    if (e != hipSuccess) {  // not passed yet -- or not knowable (an error): the blocks stay lent rather than be re-used under a kernel
      (void)hipGetLastError();
      i++;
      continue;
    }
    (void)hipEventDestroy(b.done);
    for (void* p : b.bufs) (void)heap_free(p);
    c->dsync_deferred.erase(c->dsync_deferred.begin() + (long)i);
  }
}

// blocks that kernels enqueued so far may still use go back once the stream has passed them (reap_deferred) -- or, when no event
// can be recorded behind them, at finalize (dsync_leaked): never while a kernel may still use them
static hipError_t give_back_behind(xmpi_comm* c, hipStream_t stream, std::vector<void*> bufs) {
  if (bufs.empty()) return hipSuccess;
  xmpi_comm::DsyncDeferred d{nullptr, std::move(bufs)};
  hipError_t e = hipEventCreateWithFlags(&d.done, hipEventDisableTiming);
  if (e == hipSuccess && (e = hipEventRecord(d.done, stream)) != hipSuccess) (void)hipEventDestroy(d.done);
  if (e == hipSuccess) {
    c->dsync_deferred.push_back(std::move(d));
  } else {
    (void)hipGetLastError();
    c->dsync_leaked.insert(c->dsync_leaked.end(), d.bufs.begin(), d.bufs.end());
  }
  return e;
}

// a block of the registered arenas standing in for memory the peers cannot map: lent (into `lent`, whose owner gives it back) and
// exported.  nullptr: *rc says why.  The copy in -- and what a failed one means -- is the caller's.
void* lend_standin(xmpi_comm* c, std::vector<void*>& lent, size_t bytes, BufRef* ref, int* rc) {
  void* p = heap_alloc(c->device, bytes);
  if (!p) {
    *rc = XMPI_ERR_NOMEM;
    return nullptr;
  }
  lent.push_back(p);
  if (!zc_export(c, p, bytes, ref)) {
    *rc = XMPI_ERR_HIP;
    return nullptr;
  }
  c->dsync_bounced++;
  return p;
}

// a capture bakes addresses into the graph: a stand-in would be given back to the arena while replays still use it
int capture_needs_registered() {
  set_last_error("graph capture needs registered device buffers (xmpi_malloc / xmpi_register)");
  return XMPI_ERR_ARG;
}

// pinned memory for the host slices of blocking collectives; false = not available (the runtime's own staged copies serve)
bool host_bounce_ready(xmpi_comm* c) {
  if (c->host_bounce_dev) return true;
  if (c->host_bounce) return false;  // tried before
  void* p = nullptr;
  if (hipHostMalloc(&p, 2 * xmpi_comm::kHostBounce, hipHostMallocMapped) != hipSuccess) {
    (void)hipGetLastError();
    c->host_bounce = reinterpret_cast<char*>(1);  // remember the failure
    return false;
  }
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipHostFree(p);
    c->host_bounce = reinterpret_cast<char*>(1);
    return false;
  }
  c->host_bounce = (char*)p;
  c->host_bounce_dev = (char*)dev;
  return true;
}

// one launch of the copy-and-flag kernel (sched.hip p2p_pull_kernel) between a stand-in and the pinned memory above
hipError_t bounce_copy(xmpi_comm* c, void* dst, const void* src, size_t bytes, int which, uint64_t* done, uint64_t done_value, hipStream_t s) {
  P2PPullArgs pa;
  memset(&pa, 0, sizeof pa);
  pa.dst = dst;
  pa.src = src;
  pa.bytes = bytes;
  pa.ticket = c->p2p_tickets + xmpi_comm::kP2PDoneSlots + which;
  pa.host_done = done;
  pa.done_value = done_value;
  const long gx = std::max<long>(1, std::min<long>(16, (long)((bytes + 16383) >> 14)));
  return launch_p2p_pull(pa, (int)gx, s);
}

// A blocking call waits for its stream (polling: the wake-up latency of hipStreamSynchronize is a visible share of a small
// collective), serving the peers meanwhile.  by_word: the closing block of the (last) kernel writes the call's number into a
// pinned word (dsync_status bytes 16..23): no event between the kernel and this thread.  (The kernel itself gives up on a
// dead peer -- abort flag, XMPI_TIMEOUT_S -- and still writes the word.)
static int wait_blocking(xmpi_comm* c, hipStream_t stream, bool by_word, uint64_t done_id) {
  Backoff bo;
  arm(bo, c);
  if (by_word) {
    const volatile uint64_t* done = (const volatile uint64_t*)(c->dsync_status + 4);
    // Safety valve, off the fast path: once the wait is long, ask the stream now and then -- a stream that is idle (or broken)
    // while the word is still missing must not hang the caller.
    unsigned spins = 0;
    while (__atomic_load_n((const uint64_t*)done, __ATOMIC_ACQUIRE) != done_id) {
      bo.pause();
      if ((++spins & 0x3fff) == 0) {
        const hipError_t e = hipStreamQuery(stream);
        if (e == hipErrorNotReady) {
          (void)hipGetLastError();
          continue;
        }
        if (e != hipSuccess) return hip_fail(e, "hipStreamQuery", __FILE__, __LINE__);
        if (__atomic_load_n((const uint64_t*)done, __ATOMIC_ACQUIRE) != done_id) {
          set_last_error("collective: the stream drained but the closing block never reported (internal)");
          return XMPI_ERR_STATE;
        }
      }
    }
    return XMPI_OK;
  }
  hipEvent_t fin = ev_get(c, false);
  if (!fin) return XMPI_ERR_HIP;
  XMPI_HIP(hipEventRecord(fin, stream));
  for (;;) {
    const hipError_t e = hipEventQuery(fin);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery", __FILE__, __LINE__);
    (void)hipGetLastError();
    bo.pause();
  }
  ev_put(c, fin, false);
  return XMPI_OK;
}

// ---- DsyncCall (dsync.h): what one collective borrows, and the three ways it gives it back

// the kernels of one rank share the page's epoch counter, ticket and slots: one at a time.  On one stream that is
// stream order; a launch on another stream than the previous one waits for it.
// (The event is recorded when the stream CHANGES, at the tail of the previous stream -- not behind every launch: an event
// per collective costs the queue a packet and was visible in the small-message figures.)
int DsyncCall::order_behind_last() {
  if (capturing || !c->dsync_last_stream || c->dsync_last_stream == stream) return XMPI_OK;
  hipStreamCaptureStatus pc = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(c->dsync_last_stream, &pc);
  (void)hipGetLastError();
  if (pc == hipStreamCaptureStatusNone) {  // (a capturing stream runs nothing until its graph is launched: dsync_graph_launched)
    XMPI_HIP(hipEventRecord(c->dsync_order_ev, c->dsync_last_stream));
    XMPI_HIP(hipStreamWaitEvent(stream, c->dsync_order_ev, 0));
  }
  return XMPI_OK;
}

// how every call opens: the peers are served, blocks lent to calls the streams have passed since are taken back, and the stream is
// asked whether it captures
static bool open_call(xmpi_comm* c, hipStream_t stream) {
  dsync_service(c);
  reap_deferred(c, false);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream, &cap);
  (void)hipGetLastError();
  return cap != hipStreamCaptureStatusNone;
}

// (`calls` -- t_api_call -- is read before open_call serves the peers: the members are initialised in the order dsync.h declares them)
DsyncCall::DsyncCall(xmpi_comm* comm, hipStream_t s, bool b)
    : c(comm), stream(s ? s : comm->local_stream), blocking(b), capturing(open_call(comm, stream)) {}

void* DsyncCall::lend(size_t bytes) {
  void* p = heap_alloc(c->device, bytes);
  if (p) lent.push_back(p);
  return p;
}

// The communicator KEEPS one registered block for what a stepped collective needs beside the caller's buffers -- the push forms'
// landing block, the pull-form tree reduce's accumulator -- and uses it again for the next one (grown when one needs more): the
// peers touch it only between this rank's announce for a collective and its close, and its kernels run one at a time -- so
// back-to-back enqueued collectives share one block, where a block lent per call would have each of them take a new one before
// the stream has given the last one back (1 GiB fp16, halving push form, 5 enqueued steps: a new 1 GiB arena allocated,
// exported and mapped by every peer per step -- 100 ms instead of 9).
void* DsyncCall::own_block(size_t bytes) {
  if (!c->land_block || c->land_block_bytes < bytes) {
    // the outgrown block goes back once THIS collective's kernel -- behind every earlier one -- has passed.  Not through `lent`:
    // a failure gives `lent` back at once, and earlier ENQUEUED collectives may still be landing in this block
    if (c->land_block) outgrown = c->land_block;
    c->land_block = heap_alloc(c->device, bytes);
    c->land_block_bytes = c->land_block ? bytes : 0;
  }
  return c->land_block;
}

// behind order_behind_last, before the first launch: the call's number, and whether its launches are sampled
void DsyncCall::begin() {
  done_id = ++c->dsync_done_seq;
  done_dev = (blocking && c->dsync_status_dev) ? (uint64_t*)(c->dsync_status_dev + 4) : nullptr;
  sampled = !capturing && c->prof_on && (c->prof_seq[PROF_ZCOPY]++ % (uint64_t)std::max<long>(1, c->prof_every)) == 0;
}

// sampled launches carry their own begin / end events (attached to the dispatch); a launch that is only enqueued
// leaves them for the next blocking call to read, so sampling does not put a host wait between enqueued steps
bool DsyncCall::prof_events() {
  if (sampled && !pstart) {
    pstart = ev_get(c, true);
    pstop = ev_get(c, true);
    if (!pstart || !pstop) return false;
  }
  return true;
}

void DsyncCall::keep_prof() {
  if (pstart) c->dsync_prof_pending.push_back({pstart, pstop, traffic});
  pstart = pstop = nullptr;
}

// a failure once blocks are borrowed or the epoch has advanced: the stand-ins go back at once, the outgrown block behind what
// the stream holds, and the peers -- whose kernels would wait for this rank -- are told through the job's abort flag
int DsyncCall::fail(int rc) {
  for (void* p : lent) (void)heap_free(p);
  lent.clear();
  if (outgrown) (void)give_back_behind(c, stream, {outgrown});
  outgrown = nullptr;
  c->ctl->set_abort(rc);
  return rc;
}

// The result of a stand-in goes home, the blocks go back.  (A copy into pageable host memory blocks the calling thread until
// the kernel before it has ended -- and the kernel ends only when every peer has arrived, which a peer may be unable to do
// before THIS rank has mapped a buffer it just registered.  So a blocking call copies out after its polling wait, which serves
// the peers; the stream-ordered forms take device memory only, where the copy really is asynchronous.)
int DsyncCall::enqueued(void* home, size_t bytes) {
  keep_prof();
  if (out_src) {
    const hipError_t e = hipMemcpyAsync(home, out_src, bytes, hipMemcpyDefault, stream);
    if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpyAsync(result of a stand-in)", __FILE__, __LINE__));
  }
  if (outgrown) lent.push_back(outgrown);
  outgrown = nullptr;
  const hipError_t e = give_back_behind(c, stream, std::move(lent));
  lent.clear();
  return e == hipSuccess ? XMPI_OK : fail(hip_fail(e, "hipEventRecord(blocks lent to an enqueued collective)", __FILE__, __LINE__));
}

int DsyncCall::wait_and_finish(void* home, size_t bytes) {
  const int rc = wait_blocking(c, stream, done_dev != nullptr, done_id);
  if (rc != XMPI_OK) return fail(rc);
  // (the kernel's last act was the word this call waited for; everything before it on the streams is over -- unless another
  // thread has entered the library meanwhile.  The next blocking small collective need not ask the streams: dsync_ll)
  if (c->api_calls.load(std::memory_order_relaxed) == calls) c->agent_quiet_at = calls;
  if (outgrown) lent.push_back(outgrown);  // (the stream has passed this collective, and with it every earlier one)
  outgrown = nullptr;
  if (host_out) {
    memcpy(home, c->host_bounce + xmpi_comm::kHostBounce, bytes);
  } else if (out_src) {
    hipError_t e = hipMemcpyAsync(home, out_src, bytes, hipMemcpyDefault, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(hip_fail(e, "copy of a stand-in's result", __FILE__, __LINE__));
  }
  for (void* p : lent) (void)heap_free(p);
  lent.clear();
  keep_prof();
  dsync_prof_harvest(c);
  return dsync_check(c);
}

// hipGraphLaunch of a captured sequence of collectives is a device-synchronised launch like any other: it is ordered
// against the rank's other streams (before = true: ahead of the launch; false: behind it)
void dsync_graph_launched(xmpi_comm* c, hipStream_t stream, bool before) {
  if (!c->dsync_ok || !c->dsync_order_ev) return;
  if (before) {
    if (c->dsync_last_stream && c->dsync_last_stream != stream) {
      (void)hipEventRecord(c->dsync_order_ev, c->dsync_last_stream);
      (void)hipStreamWaitEvent(stream, c->dsync_order_ev, 0);
    }
  } else {
    c->dsync_last_stream = stream;
  }
  (void)hipGetLastError();
}

// the events of sampled launches that have ended (a launch that was only enqueued leaves them for a later look) go into
// the profile counters
void dsync_prof_harvest(xmpi_comm* c) {
  for (size_t i = 0; i < c->dsync_prof_pending.size();) {
    auto& p = c->dsync_prof_pending[i];
    float ms = 0.f;
    if (hipEventQuery(p.stop) != hipSuccess || hipEventElapsedTime(&ms, p.start, p.stop) != hipSuccess) {
      (void)hipGetLastError();
      i++;
      continue;
    }
    ProfCounter& pc = c->prof[PROF_ZCOPY];
    pc.add(ms, p.bytes);
    ev_put(c, p.start, true);
    ev_put(c, p.stop, true);
    c->dsync_prof_pending.erase(c->dsync_prof_pending.begin() + (long)i);
  }
}

// the first failure a kernel of this rank reported since the last look (a wait that was cut short, a buffer
// reference it could not translate); clears it
int dsync_check(xmpi_comm* c) {
  if (!c->dsync_status) return XMPI_OK;
  const uint32_t st = __atomic_exchange_n(c->dsync_status, 0u, __ATOMIC_ACQ_REL);
  // xmpi_alltoallv's own verdicts (DsyncVStatus, word 13): one pair's business -- the job is NOT aborted, the communicator stays
  // usable, as after a truncated xmpi_recv; a timeout or an abort in the same kernel is what gets reported
  const uint32_t vst = __atomic_exchange_n(c->dsync_status + 13, 0u, __ATOMIC_ACQ_REL);
  if (st == DSYNC_OK && vst != 0) {
    const std::string peer = std::to_string((int)(vst >> 8) - 1);
    if ((vst & 0xffu) == DSYNC_BOUNDS) {
      set_last_error("alltoallv: the arrays' row for rank " + peer + " leaves the extents of the buffers; nothing was moved between the two");
      return XMPI_ERR_ARG;
    }
    set_last_error("alltoallv: the block exchanged with rank " + peer + " is longer than the capacity its receiver granted; it was not moved");
    return XMPI_ERR_TRUNCATE;
  }
  if (st == DSYNC_OK) return XMPI_OK;
  int rc = XMPI_ERR_PEER;
  if (st == DSYNC_TIMEOUT) {
    set_last_error("collective: a peer did not arrive within XMPI_TIMEOUT_S (kernel wait cut short)");
    rc = XMPI_ERR_TIMEOUT;
  } else if (st == DSYNC_UNMAPPED) {
    set_last_error("collective: a peer's buffer is not mapped here (registration freed while in use?)");
    rc = XMPI_ERR_STATE;
  } else if (st == DSYNC_MISMATCH) {
    set_last_error("collective: the ranks are not in the same call (collective, schedule, length, dtype, operation or root differ "
                   "between this rank and a peer); nothing was moved");
    rc = XMPI_ERR_ARG;
  } else if (st == DSYNC_XCD) {
    c->xcd_short++;
    set_last_error("collective: the meet / done kernels of the split form did not reach every XCD's L2 (masks in xcd_meet_mask / "
                   "xcd_done_mask); set XMPI_BODY_SYS=1");
    rc = XMPI_ERR_STATE;
  } else {
    set_last_error("collective: the job was aborted while the kernel waited for a peer: " + c->ctl->abort_reason());
  }
  c->ctl->set_abort(rc);
  return rc;
}

}  // namespace xmpi
