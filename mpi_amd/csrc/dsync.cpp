// dsync.cpp -- device-synchronised, stream-ordered collectives.
//
// The zero-copy collectives of zcopy.cpp meet on the HOST: two or three barriers through the shared control
// block around every kernel.  Here the ranks meet on the DEVICE: each rank owns a flag page in its HBM
// (uncached, mapped by every peer), and one kernel per rank (kernels.hip `dsync_fold_kernel`) announces this
// rank's buffers to the peers, waits for theirs, moves the data straight between the user buffers over xGMI
// and exchanges "done" before it ends.  The host only enqueues that kernel on a stream -- its own for the
// blocking calls (xmpi_allreduce ...), the caller's for xmpi_*_on_stream -- and never polls a peer: what the
// reference does with a message + ack over a net.Conn per Send (network.go:562-571) is two 8-byte stores
// over a link here.
//
// What still needs the host, rarely: a kernel can only address a peer's buffer through a mapping (hipIpc)
// this process has opened.  Every rank therefore PUBLISHES the allocations it registers (control block,
// PubTable), every peer maps them the next time it is inside the library (`dsync_service`, also called from
// every wait loop), writes {slot -> mapping} into the translation table its kernels read, and acknowledges.
// A rank uses a buffer in a device-synchronised collective only after all peers acknowledged the allocation
// it lives in: in steady state (buffers allocated once, reused) nothing of this runs.
//
// Applies when no two ranks share a (process, GPU) pair -- the production layout, one process per MI355X.
// Ranks hosted by threads of one process on one GPU (bench.py on a single-GPU box) keep the host-synchronised
// path: they share one in-order stream, and a kernel that waits for a kernel queued behind it never ends.
//
// Six collectives are segment lists over the same kernels (DsyncSeg: whose buffers a block reads, whose it writes).  Reduce-scatter and
// all-to-all cut their buffers into BLOCKS of count elements, which -- unlike the 16-byte aligned chunks the others are cut into
// (zc_chunk) -- start wherever me x count x element size falls: blocks that are a multiple of 16 bytes take the fold kernel's
// packet path, any other length its one-element-per-lane path (correct, slow).
//
// The connection lifecycle (dsync_prepare / dsync_connect / the helper thread / dsync_finalize) and dsync_service: dsync_conn.cpp.
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "comm.h"
#include "kernels.h"
#include "sched_steps.h"

namespace xmpi {

static_assert(kDsyncRanks <= kMaxRanks, "the device side serves a subset of the jobs the host side admits");

namespace {

void idle_hook(void* arg) { dsync_service((xmpi_comm*)arg); }

// the slot of my translation-table row that holds registration `gen`; publishes it if need be.
// *pub_index = how many published entries a peer must have processed to know it.
int publish(xmpi_comm* c, const BufRef& ref, int* slot_out, uint64_t* pub_index, bool capturing = false) {
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
  bo.idle = idle_hook;
  bo.idle_arg = c;
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

int await_acks(xmpi_comm* c, uint64_t pub_index) {
  Backoff bo;
  bo.idle = idle_hook;
  bo.idle_arg = c;
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
void reap_deferred(xmpi_comm* c, bool wait) {
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
hipError_t give_back_behind(xmpi_comm* c, hipStream_t stream, std::vector<void*> bufs) {
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

struct Resolved {
  const void* send = nullptr;
  void* recv = nullptr;
  BufRef sref, rref;
  void* tmp_send = nullptr;  // registered stand-ins of buffers the peers cannot map
  void* tmp_recv = nullptr;
};

// a collective's arguments, as its steps read them
struct CollArgs {
  int coll, root, dtype, op;
  size_t count, es;               // elements per rank (reduce-scatter, all-to-all: per block), bytes per element
  size_t unit;                    // count x es: the message, or -- reduce-scatter, all-to-all -- the block one rank gives one peer
  size_t send_bytes, recv_bytes;  // what the buffers hold (plan.h coll_send_bytes / coll_recv_bytes)
};

// pinned memory for the host slices of blocking collectives; false = not available (the runtime's own staged copies serve)
static bool host_bounce_ready(xmpi_comm* c) {
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
static hipError_t bounce_copy(xmpi_comm* c, void* dst, const void* src, size_t bytes, int which, uint64_t* done, uint64_t done_value,
                              hipStream_t s) {
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
  bo.idle = idle_hook;
  bo.idle_arg = c;
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

// the kernels of one rank share the page's epoch counter, ticket and slots: one at a time.  On one stream that is
// stream order; a launch on another stream than the previous one waits for it.
// (The event is recorded when the stream CHANGES, at the tail of the previous stream -- not behind every launch: an event
// per collective costs the queue a packet and was visible in the small-message figures.)
static int order_behind_last(xmpi_comm* c, hipStream_t stream, bool capturing) {
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

// What one collective borrows -- stand-ins lent from the registered arenas, the landing block it outgrew, the sampled events, the
// done word -- and the three ways it gives them back: fail (nothing more runs for it), enqueued (the stream gives the blocks back
// once it has passed the call) and wait_and_finish (a blocking call's tail).
struct DsyncCall {
  xmpi_comm* const c;
  const hipStream_t stream;
  const bool blocking;
  // THIS call's number (what its XMPI_ENTER drew), not the counter as it stands now: another thread of the communicator may have
  // entered since -- it waits for coll_mu, is counted already, and what it goes on to enqueue is not this call's to vouch for
  const uint64_t calls = t_api_call;
  std::vector<void*> lent;        // stand-ins
  void* outgrown = nullptr;       // the landing block own_block replaced (one per call at most)
  bool sampled = false;           // the launches carry begin / end events ...
  hipEvent_t pstart = nullptr, pstop = nullptr;
  size_t traffic = 0;             // ... and the profile counts this many bytes for them
  uint64_t done_id = 0;           // the call's number in the done word ...
  uint64_t* done_dev = nullptr;   // ... which its closing block writes when the call blocks (dsync_status bytes 16..23)
  const void* out_src = nullptr;  // a stand-in whose contents go home to the caller's receive buffer ...
  bool host_out = false;          // ... or: the result lies in the pinned block (host_bounce, second half)

  DsyncCall(xmpi_comm* comm, hipStream_t s, bool b) : c(comm), stream(s), blocking(b) {}

  void* lend(size_t bytes) {
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
  void* own_block(size_t bytes) {
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
  void begin(bool capturing) {
    done_id = ++c->dsync_done_seq;
    done_dev = (blocking && c->dsync_status_dev) ? (uint64_t*)(c->dsync_status_dev + 4) : nullptr;
    sampled = !capturing && c->prof_on && (c->prof_seq[PROF_ZCOPY]++ % (uint64_t)std::max<long>(1, c->prof_every)) == 0;
  }

  // sampled launches carry their own begin / end events (attached to the dispatch); a launch that is only enqueued
  // leaves them for the next blocking call to read, so sampling does not put a host wait between enqueued steps
  bool prof_events() {
    if (sampled && !pstart) {
      pstart = ev_get(c, true);
      pstop = ev_get(c, true);
      if (!pstart || !pstop) return false;
    }
    return true;
  }
  void keep_prof() {
    if (pstart) c->dsync_prof_pending.push_back({pstart, pstop, traffic});
    pstart = pstop = nullptr;
  }

  // a failure once blocks are borrowed or the epoch has advanced: the stand-ins go back at once, the outgrown block behind what
  // the stream holds, and the peers -- whose kernels would wait for this rank -- are told through the job's abort flag
  int fail(int rc) {
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
  int enqueued(void* home, size_t bytes) {
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

  int wait_and_finish(void* home, size_t bytes) {
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
};

}  // namespace

// ---- LL small collectives (ll.hip): the payload is pushed into the peers' flag allocations, nothing is registered,
// announced or translated; one kernel, one one-way hop.  Whether a call goes this way is decided by dsync_collective from the
// arguments and the job's layout only (the same on every rank); what kind of memory a rank passes is this rank's business.
static int dsync_ll(DsyncCall& call, const CollArgs& k, const void* sendbuf, void* recvbuf, bool capturing) {
  xmpi_comm* const c = call.c;
  const hipStream_t stream = call.stream;
  const bool blocking = call.blocking;
  const int N = c->size, me = c->rank, coll = k.coll, root = k.root;
  const size_t unit = k.unit, send_bytes = k.send_bytes, recv_bytes = k.recv_bytes;
  RoctxRange range("xmpi:dsync %s form=ll bytes=%zu epoch=%llu %s", coll_name(coll), unit, (unsigned long long)c->dsync_epoch + 1,
                   blocking ? "blocking" : "enqueued");
  const bool reads = coll != COLL_BCAST || me == root;           // this rank's send buffer is read
  const bool writes = (coll != COLL_REDUCE || me == root) && !(coll == COLL_BCAST && me == root);  // its receive buffer is written
  auto on_gpu = [&](const void* p, size_t bytes) {
    BufRef ref;
    return zc_export(c, p, bytes, &ref) || is_device_pointer(p);
  };
  const void* send = sendbuf;
  void* recv = recvbuf;
  // a host slice: through pinned memory the kernel reads / writes itself, or a stand-in
  const bool host_in = reads && !on_gpu(sendbuf, send_bytes), host_res = writes && !on_gpu(recvbuf, recv_bytes);
  if (capturing && (host_in || host_res)) {
    set_last_error("graph capture needs device buffers");
    return XMPI_ERR_ARG;
  }
  if (host_in) {
    if (blocking && send_bytes <= xmpi_comm::kHostBounce && host_bounce_ready(c)) {
      memcpy(c->host_bounce, sendbuf, send_bytes);
      send = c->host_bounce_dev;
      c->host_bounce_calls++;
    } else {
      void* tmp = call.lend(send_bytes);
      if (!tmp) return call.fail(XMPI_ERR_NOMEM);
      const hipError_t ce = hipMemcpyAsync(tmp, sendbuf, send_bytes, hipMemcpyDefault, stream);
      if (ce != hipSuccess) return call.fail(hip_fail(ce, "hipMemcpyAsync(stand-in)", __FILE__, __LINE__));
      send = tmp;
    }
  }
  if (host_res) {
    if (blocking && recv_bytes <= xmpi_comm::kHostBounce && c->dsync_status_dev && host_bounce_ready(c)) {
      recv = c->host_bounce_dev + xmpi_comm::kHostBounce;
      call.host_out = true;
      c->host_bounce_calls++;
    } else {
      recv = call.lend(recv_bytes);
      if (!recv) return call.fail(XMPI_ERR_NOMEM);
      call.out_src = recv;
    }
  }
  if (!writes) recv = const_cast<void*>(send);  // (never written; the launcher wants a pointer)
  if (!reads) send = recv;
  const int ll_coll = coll == COLL_ALLREDUCE ? LL_ALLREDUCE : coll == COLL_REDUCE ? LL_REDUCE : coll == COLL_BCAST ? LL_BCAST
                      : coll == COLL_ALLGATHER ? LL_ALLGATHER : coll == COLL_REDUCE_SCATTER ? LL_REDUCE_SCATTER : LL_ALLTOALL;
  // A blocking call -- the only kind the reference's API has (mpi.go:47-48) -- is launch + kernel + completion word, and the
  // launch is half of it.  The LL agent (ll.hip ll_agent_kernel: a one-block kernel that lingers behind the previous blocking small
  // collective, as the receive agent does behind a Receive) runs the same lines without one: the command goes through pinned
  // memory, the answer comes back the same way.  Only when the stream the call would have
  // been enqueued on is idle and nothing this communicator enqueued elsewhere is still running (the agent cannot wait for a
  // stream; the launched kernel is ordered behind both), nothing is being profiled per dispatch, and no stand-in needs a copy
  // on the stream first.
  // (the streams are not asked when the previous call into the library on this communicator was itself a collective the agent
  // ran: it found them idle, and nothing has been enqueued through the library since)
  const uint64_t calls = call.calls;
  auto idle = [](hipStream_t s) { return hipStreamQuery(s) == hipSuccess; };
  const bool quiet = calls == c->agent_quiet_at + 1, consecutive = calls == c->agent_epoch_at + 1;
  // up to agent_ll_bytes (8 KiB: a lane's two rounds of lines are waited for together -- blocking 8.8 us against 11.7 launched,
  // 2 processes; host slices 10.0 against 13.8; at 16 KiB it is a tie, 12.1 / 11.7, and beyond the launched kernel's many blocks
  // win) -- scripts/r04_agent_limit.sh
  const size_t agent_limit = (size_t)std::max<long>(0, c->agent_ll_bytes);
  // (the agent knows the four collectives whose ranks all send the same line; reduce-scatter and all-to-all are launched)
  if (blocking && !capturing && !coll_personal(coll) && call.lent.empty() && c->agent_ll && unit <= agent_limit && !c->prof_on &&
      (quiet ||
       (idle(stream) && (!c->dsync_last_stream || c->dsync_last_stream == stream || idle(c->dsync_last_stream))))) {
    ++c->dsync_epoch;
    const double t_cmd = now_seconds();
    // An agent that has gone is started again, whatever the caller's pace.  Tried and measured (scripts/r04_agent_patience.sh, 2
    // processes, 1 KiB, the caller's own work between two calls 100 / 500 us, patience 40): starting it only for a BURST of calls --
    // the previous one less than a patience ago -- and launching the ordinary kernel otherwise: 25.4 / 25.3 us per call, against
    // 14.4 / 21.5 with the agent started by every call (a launch into a GPU that has been idle for 100 us costs more than one into a
    // busy GPU; the agent's launch overlaps with the command already lying in its record) and 7.5 inside its patience.
    const int took = agent_submit_ll(c, send, recv, unit, ll_coll, root, k.dtype, k.op, consecutive);
    if (took < 0) {  // taken and never answered: the collective has failed, nothing may run for this epoch beside the agent
      set_last_error("collective: the LL agent did not answer within XMPI_TIMEOUT_S (a peer that never arrived?)");
      return call.fail(XMPI_ERR_TIMEOUT);
    }
    if (took > 0) {
      c->agent_ll_wait_ns += (uint64_t)((now_seconds() - t_cmd) * 1e9);
      // (only when no other thread has entered the library on this communicator meanwhile: what it goes on to enqueue is not
      // this call's to vouch for)
      if (c->api_calls.load(std::memory_order_relaxed) == calls) c->agent_quiet_at = c->agent_epoch_at = calls;
      c->dsync_ll_launches++;  // (an LL collective, whoever ran its lines)
      c->dsync_ll_agent++;
      if (call.host_out) memcpy(recvbuf, c->host_bounce + xmpi_comm::kHostBounce, recv_bytes);
      return dsync_check(c);
    }
    --c->dsync_epoch;
  }
  (void)hipGetLastError();
  const int rc = order_behind_last(c, stream, capturing);
  if (rc != XMPI_OK) return call.fail(rc);
  call.begin(capturing);

  DsyncLLArgs a;
  memset(&a, 0, sizeof a);
  for (int p = 0; p < N; p++) a.page[p] = c->peer_page[p];
  a.me = me;
  a.n = N;
  a.coll = ll_coll;
  a.root = root;
  a.epoch_floor = c->dsync_base;
  a.host_epoch = c->dsync_status_dev ? (uint64_t*)(c->dsync_status_dev + 2) : nullptr;
  a.host_done = call.done_dev;
  a.done_value = call.done_id;
  a.send = send;
  a.recv = recv;
  a.bytes = unit;
  a.abort_word = c->dsync_abort_dev;
  a.status = c->dsync_status_dev;
  a.spin_limit = c->timeout_s > 0 ? (uint64_t)c->timeout_s * 100000000ull : 0;
  if (!call.prof_events()) return call.fail(XMPI_ERR_HIP);
  ++c->dsync_epoch;
  {
    const hipError_t le = launch_dsync_ll(a, k.dtype, k.op, stream, call.pstart, call.pstop);
    if (le != hipSuccess) {  // nothing was enqueued: the host's count goes back, the lent blocks too, and the peers -- whose kernels
      --c->dsync_epoch;      // wait for this rank's lines -- are told through the job's abort flag (fail)
      return call.fail(hip_fail(le, "LL kernel launch", __FILE__, __LINE__));
    }
  }
  c->dsync_launches++;
  c->dsync_ll_launches++;
  if (!capturing) c->dsync_last_stream = stream;
  call.traffic = 2 * unit * (size_t)N;  // (own payload read -- reduce-scatter, all-to-all: a block per peer --, N-1 pushes of twice its size ... : a latency path, not a bandwidth one)
  call.keep_prof();
  return blocking ? call.wait_and_finish(recvbuf, recv_bytes) : call.enqueued(recvbuf, recv_bytes);
}

bool dsync_usable(const xmpi_comm* c) { return c->dsync_ok && c->dsync && c->size > 1; }

// blocks a kernel of this rank may keep waiting at once: the kernels of all ranks on one GPU spin together, so with
// several ranks per GPU they must all be resident (half of its 8192 wave slots, 4 waves per block, shared)
static long dsync_block_cap(const xmpi_comm* c) {
  if (c->dsync_grid_cap > 0) return c->dsync_grid_cap;
  // (a rank alone on its GPU keeps to half of the chip too: while its blocks wait for a late peer the caller's other streams
  // still find wave slots -- scripts/overlap_probe.hip: a full-chip compute kernel next to a waiting 1024-block collective
  // runs 5 % slower, next to the meet / body / done form 1.5 %)
  // (Eight processes on one GPU, 64 instead of 128 blocks per rank: 6 % faster at 256 MiB on one box, 12 % slower on the next --
  // scripts/r03_tiles.sh; XMPI_DSYNC_GRID=256 per rank = every wave slot of the chip: the kernels wait for each other for ever.)
  return 1024 / std::max(1, c->dsync_sharers);
}

int dsync_grid(const xmpi_comm* c, size_t packets_per_segment, int nseg, int unroll) {
  long cap = std::max<long>(1, dsync_block_cap(c) / std::max(1, nseg));
  // several tiles per block: every block costs seven polling lanes on this rank's page and a ticket, which is what a
  // small collective spends its time on (8 processes, 1 MiB: 32 blocks per rank -> 84 us, see profiles/README.md)
  const size_t per_block = (size_t)256 * (size_t)std::max(1, unroll) * (size_t)std::max<long>(1, c->dsync_tiles);
  const size_t want = (packets_per_segment + per_block - 1) / per_block;
  return (int)std::max<size_t>(1, std::min<size_t>(want, (size_t)cap));
}

// which calls the device-synchronised path takes (the same answer on every rank: it depends on the job's layout
// and the arguments only)
bool dsync_takes(const xmpi_comm* c, int coll, int algo) {
  if (!dsync_usable(c)) return false;
  if (!c->windows_ok) return true;  // a job without windows has no staged step tables: DIRECT and whatever else names them is the fold
  switch (algo) {
    case XMPI_ALGO_AUTO: return c->zero_copy != 0;
    case XMPI_ALGO_ZCOPY:
    case XMPI_ALGO_ZPUSH:
    case XMPI_ALGO_LL: return true;
    case XMPI_ALGO_RING:  // the stepped kernels (sched.hip), pull and push form
    case XMPI_ALGO_RING_PUSH: return coll == COLL_ALLREDUCE || coll == COLL_ALLGATHER;
    case XMPI_ALGO_RHD:
    case XMPI_ALGO_RHD_PUSH: return coll == COLL_ALLREDUCE;
    case XMPI_ALGO_TREE:
    case XMPI_ALGO_TREE_PUSH: return coll == COLL_BCAST || coll == COLL_REDUCE;
    default: return false;
  }
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

namespace {

struct DsyncRoute {
  enum Form { LL, FOLD, PUSH_ONLY, STEPPED } form = FOLD;  // FOLD: one kernel or meet / body / done (bcast and allgather: theirs)
  int algo = XMPI_ALGO_AUTO;        // the schedule as it runs: after the table and the capture demotions
  int sched_algo = XMPI_ALGO_AUTO;  // ... a stepped kernel by its pull form's name (RING, RHD, TREE)
  bool sched_push = false;          // ... and whether it pushes
  int split_pref = -1;              // one kernel (0) or meet / body / done (1); -1: by size (dsync_split_bytes)
  int unroll = 1;
  int refused = -1;                 // the rejected candidate (xmpi_comm::CAND_*) the caller named: nothing runs; -1: none
};

// From the communicator and the arguments only -- the same answer on every rank, so every rank refuses alike, hands the same calls
// to LL and launches the same form.  Pure: no HIP, no counters, no error text.
// unit: the message -- reduce-scatter, all-to-all: the BLOCK, which is what a slot of LL lines has to hold and what every link carries
DsyncRoute dsync_route(const xmpi_comm* c, int coll, int algo, size_t unit, bool capturing) {
  DsyncRoute rt;
  rt.unroll = (int)std::max<long>(1, std::min<long>(2, c->dsync_unroll));
  // the schedule: what the caller named, or the library's own table (xmpi_tune fills it; untuned: the zero-copy fold, split by size)
  if (algo == XMPI_ALGO_AUTO) {
    int cls = 0;
    while (cls + 1 < xmpi_comm::kTuneClasses && (unit >> (cls + 9)) != 0) cls++;
    if (c->tuned && coll >= 0 && coll < kTunedColls) {
      if (c->tune_algo[coll][cls] >= 0) algo = c->tune_algo[coll][cls];
      if (c->tune_split[coll][cls] >= 0) rt.split_pref = c->tune_split[coll][cls];
      if (c->tune_unroll[coll][cls] > 0) rt.unroll = c->tune_unroll[coll][cls];
    }
    // untuned: short messages go as {data, flag} lines (ll.hip) -- one one-way hop instead of two round trips
    if (algo == XMPI_ALGO_AUTO && c->zero_copy && unit <= (size_t)std::max<long>(0, c->ll_bytes)) algo = XMPI_ALGO_LL;
  }
  // A schedule whose ANSWERS xmpi_tune or xmpi_init's self-check found wrong on this machine (tune_rejected: the outcome of a vote,
  // the same bits on every rank) is not run for a caller: AUTO never leads here (the table leaves it out, apply_rejections the untuned
  // rules), so this is a caller -- or a table written by hand -- naming it.  Every rank refuses alike, before anything is lent,
  // announced or moved.
  const uint32_t rejected = (c->tune_running || coll < 0 || coll >= kTunedColls) ? 0u : c->tune_rejected[coll];
  auto no = [rejected](int cand) { return ((rejected >> cand) & 1u) != 0; };
  if (algo == XMPI_ALGO_LL) {
    if (unit <= kLLMaxPayload) {
      rt.form = DsyncRoute::LL;
      rt.algo = algo;
      if (no(xmpi_comm::CAND_LL)) rt.refused = xmpi_comm::CAND_LL;
      return rt;
    }
    algo = XMPI_ALGO_ZCOPY;  // named, but too long for the slots: the fold (the same decision on every rank)
  }
  // the push forms of the stepped kernels: the same schedule, the data stored into the peer instead of loaded from it
  rt.sched_push = algo == XMPI_ALGO_RING_PUSH || algo == XMPI_ALGO_RHD_PUSH || algo == XMPI_ALGO_TREE_PUSH;
  rt.sched_algo = algo == XMPI_ALGO_RING_PUSH ? XMPI_ALGO_RING : algo == XMPI_ALGO_RHD_PUSH ? XMPI_ALGO_RHD
                  : algo == XMPI_ALGO_TREE_PUSH ? XMPI_ALGO_TREE : algo;
  if (capturing) {
    // A graph cannot hold what is lent per call -- a landing block, the tree reduce's accumulator: replays would use it after it
    // went back to the arena.  Captured, a push form runs as its pull form (the same operands, order and association: the same
    // bits) and the tree reduce as the fold -- whatever named them, the caller or the tuner's table.  Every rank captures a
    // collective or none does (as with push-only below), so every rank decides alike: by the arguments, not by what IT would lend.
    if (rt.sched_push) algo = rt.sched_algo;
    rt.sched_push = false;
    if (rt.sched_algo == XMPI_ALGO_TREE && coll == COLL_REDUCE) algo = rt.sched_algo = XMPI_ALGO_ZCOPY;
  }
  rt.algo = algo;
  const int s = rt.sched_algo;
  if ((s == XMPI_ALGO_RING && (coll == COLL_ALLREDUCE || coll == COLL_ALLGATHER)) || (s == XMPI_ALGO_RHD && coll == COLL_ALLREDUCE) ||
      (s == XMPI_ALGO_TREE && (coll == COLL_BCAST || coll == COLL_REDUCE))) {
    rt.form = DsyncRoute::STEPPED;
    const int cand = s == XMPI_ALGO_RING ? (rt.sched_push ? xmpi_comm::CAND_RING_PUSH : xmpi_comm::CAND_RING)
                     : s == XMPI_ALGO_RHD ? (rt.sched_push ? xmpi_comm::CAND_RHD_PUSH : xmpi_comm::CAND_RHD)
                                          : (rt.sched_push ? xmpi_comm::CAND_TREE_PUSH : xmpi_comm::CAND_TREE);
    if (no(cand)) rt.refused = cand;
  } else if (algo == XMPI_ALGO_ZPUSH && (coll == COLL_ALLREDUCE || coll == COLL_REDUCE || coll == COLL_REDUCE_SCATTER) && !capturing) {
    // (under capture the push-only form is the fold: its staging area is a block the communicator may replace later)
    rt.form = DsyncRoute::PUSH_ONLY;
    if (no(xmpi_comm::CAND_ZPUSH)) rt.refused = xmpi_comm::CAND_ZPUSH;
  } else if (coll == COLL_BCAST) {  // (its fold is one kernel whatever the size)
    if (no(xmpi_comm::CAND_FOLD)) rt.refused = xmpi_comm::CAND_FOLD;
  } else {
    // one kernel or meet / body / done is each rank's own choice (the two mix: dsync_begin / the meet kernel speak one protocol):
    // a rank keeps to the one of the two that is right here
    if (no(xmpi_comm::CAND_FOLD) && no(xmpi_comm::CAND_SPLIT)) rt.refused = xmpi_comm::CAND_FOLD;
    else if (no(xmpi_comm::CAND_SPLIT)) rt.split_pref = 0;
    else if (no(xmpi_comm::CAND_FOLD) && c->dsync_res) rt.split_pref = 1;
  }
  return rt;
}

int refuse(int coll, int cand) {
  set_last_error(std::string(coll_name(coll)) + " by " + xmpi_comm::kCandName[cand] + ": refused -- it gave wrong answers on this machine when "
                 "the library checked it (xmpi_get_param \"tune_rejected_" + std::to_string(coll) + "\"; xmpi_degraded() says where)");
  return XMPI_ERR_UNSUPPORTED;
}

// the call signature the kernels announce and compare (DsyncArgs::sig)
inline uint64_t sig_mix(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x100000001B3ull;
  return h ^ (h >> 29);
}
inline uint64_t sig_fold(uint64_t h) { return std::max<uint64_t>(1, (h ^ (h >> 32)) & 0xffffffffull); }

// bcast: the root stores into every buffer itself -- two ranks, or up to zc_bcast_push_bytes -- or scatters, and every rank forwards
bool bcast_forwards(const xmpi_comm* c, size_t bytes) { return c->size > 2 && bytes > (size_t)std::max<long>(0, c->zc_bcast_push_bytes); }

// What this call is, for the peers to compare with theirs (kdev.h dsync_begin): ranks that are not in the same collective, on the
// same schedule, over the same bytes end with an error before any of them has touched another's memory -- instead of a hang, or
// of a fold over buffers of different lengths.  (One kernel or meet / body / done is NOT part of it: those mix.)
uint64_t call_sig(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt) {
  const bool reduces = coll_reduces(k.coll), rooted = k.coll == COLL_BCAST || k.coll == COLL_REDUCE;
  const uint64_t form = rt.form == DsyncRoute::STEPPED ? 16u + 2u * (uint64_t)rt.sched_algo + (rt.sched_push ? 1u : 0u)
                        : rt.form == DsyncRoute::PUSH_ONLY ? 2u
                        : (k.coll == COLL_BCAST && bcast_forwards(c, k.send_bytes)) ? 3u : 1u;
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (uint64_t v : {(uint64_t)k.coll + 1, form, (uint64_t)k.send_bytes, reduces ? (uint64_t)k.dtype + 1 : 0, reduces ? (uint64_t)k.op + 1 : 0,
                     rooted ? (uint64_t)k.root + 1 : 0})
    h = sig_mix(h, v);
  return sig_fold(h);
}

// one kernel of the fold family (launch_fold: one kernel, or meet / body / done): its segments, the sources each folds (1: a copy,
// in bytes) and the bytes it moves
struct FoldStep {
  int32_t nseg = 0;
  DsyncSeg seg[kDsyncRanks] = {};
  int nsrc = 1, dtype = XMPI_U8, op = XMPI_SUM;
  size_t packets = 0, moved = 0;
  int split_pref = 0;
};
// ... a form is one or two of them, the second behind the first's close; land: the block its peers store into (0: none)
struct FoldPlan {
  FoldStep k[2];
  int kernels = 1;
  size_t land = 0;
};

uint32_t everyone(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }

// allreduce / reduce: every rank folds its chunk of everybody's send buffer, in rank order, into everybody's receive buffer (reduce:
// the root's)
FoldPlan plan_fold(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size;
  size_t off = 0, cnt = 0;
  zc_chunk(k.count, k.es, N, c->rank, &off, &cnt);
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = cnt > 0 ? 1 : 0;
  s.seg[0].src_off = s.seg[0].dst_off = off * k.es;
  s.seg[0].count = cnt;
  s.seg[0].src_mask = everyone(N);
  s.seg[0].dst_mask = k.coll == COLL_REDUCE ? (1u << k.root) : everyone(N);
  s.nsrc = N;
  s.dtype = k.dtype;
  s.op = k.op;
  s.packets = cnt / std::max<size_t>(1, 16 / k.es);
  s.moved = (size_t)(N + (k.coll == COLL_REDUCE ? 1 : N)) * cnt * k.es;
  s.split_pref = split_pref;
  return p;
}

// allgather: every rank stores its block into its place in everybody's receive buffer
FoldPlan plan_allgather(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = 1;
  s.seg[0].dst_off = (size_t)c->rank * k.send_bytes;
  s.seg[0].count = k.send_bytes;
  s.seg[0].src_mask = 1u << c->rank;
  s.seg[0].dst_mask = everyone(c->size);
  s.packets = k.send_bytes / 16;
  s.moved = (size_t)(1 + c->size) * k.send_bytes;
  s.split_pref = split_pref;
  return p;
}

// reduce-scatter: the allreduce's fold with one local destination -- every rank folds block `me` of everybody's send buffer, in rank
// order, into its own receive buffer.  Block `me` starts at me x B, which unlike a zc_chunk cut need not be 16-byte aligned:
// blocks that are a multiple of 16 bytes take the kernel's packet path, others its one-element-per-lane path (correct, slow).
FoldPlan plan_reduce_scatter(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size;
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = 1;
  s.seg[0].src_off = (size_t)c->rank * k.unit;
  s.seg[0].dst_off = 0;
  s.seg[0].count = k.count;
  s.seg[0].src_mask = everyone(N);
  s.seg[0].dst_mask = 1u << c->rank;
  s.nsrc = N;
  s.dtype = k.dtype;
  s.op = k.op;
  s.packets = k.count / std::max<size_t>(1, 16 / k.es);
  s.moved = (size_t)(N + 1) * k.unit;
  s.split_pref = split_pref;
  return p;
}

// all-to-all, push form: one segment per destination j -- my block j into place `me` of rank j's receive buffer (the own block
// is a segment like the others).  Every payload byte crosses its link as a posted store; N <= kDsyncRanks segments fit.
FoldPlan plan_alltoall(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size, me = c->rank;
  FoldPlan p;
  FoldStep& s = p.k[0];
  for (int d = 0; d < N; d++) {  // (own block first, then the next rank's: the ranks do not all store into rank 0 first)
    const int j = (me + d) % N;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = (size_t)j * k.unit;
    g.dst_off = (size_t)me * k.unit;
    g.count = k.unit;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << j;
  }
  s.packets = k.unit / 16;
  s.moved = 2 * (size_t)N * k.unit;
  s.split_pref = split_pref;
  return p;
}

// reduce-scatter, push-only (XMPI_ALGO_ZPUSH): plan_push_only below with blocks for zc_chunk's cuts -- my block q into region `me`
// of rank q's landing block, then a local fold in rank order into the receive buffer.
FoldPlan plan_reduce_scatter_push(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  const size_t region = (k.unit + 255) / 256 * 256;
  FoldPlan p;
  p.kernels = 2;
  p.land = region * (size_t)N;
  FoldStep& s = p.k[0];
  for (int d = 1; d < N; d++) {
    const int q = (me + d) % N;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = (size_t)q * k.unit;
    g.dst_off = (size_t)me * region;
    g.count = k.unit;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << q;
    g.dst_to_land = 1;
  }
  s.packets = k.unit / 16;
  s.moved = 2 * (size_t)(N - 1) * k.unit;
  p.k[1] = plan_reduce_scatter(c, k, -1).k[0];
  p.k[1].seg[0].src_from_recv = 2;
  p.k[1].seg[0].stage_stride = region;
  return p;
}

// bcast (`send` and `recv` are the same buffer on every rank), the root pushes: it stores into every buffer, the others only take
// part in the rendezvous.  (The ranks differ in what they launch: the one-kernel form, whose shape does not matter.)
FoldPlan plan_bcast_push(const xmpi_comm* c, const CollArgs& k) {
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = c->rank == k.root ? 1 : 0;
  s.seg[0].count = k.send_bytes;
  s.seg[0].src_mask = 1u << k.root;
  s.seg[0].dst_mask = everyone(c->size) & ~(1u << k.root);
  s.packets = k.send_bytes / 16;
  s.moved = c->rank == k.root ? (size_t)c->size * k.send_bytes : 0;
  return p;
}

// bcast, scatter + forward: the root scatters chunk j to rank j (one segment per destination, each over its own link), then every
// rank forwards its chunk to the others: each link carries S/N twice instead of the root's links carrying S
FoldPlan plan_bcast_forward(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  FoldPlan p;
  p.kernels = 2;
  FoldStep& s = p.k[0];
  if (me == k.root) {
    for (int j = 0; j < N; j++) {
      size_t off = 0, cnt = 0;
      zc_chunk(k.count, k.es, N, j, &off, &cnt);
      if (j == k.root || cnt == 0) continue;
      DsyncSeg& g = s.seg[s.nseg++];
      g.src_off = g.dst_off = off * k.es;
      g.count = cnt * k.es;
      g.src_mask = 1u << k.root;
      g.dst_mask = 1u << j;
      s.packets = std::max(s.packets, cnt * k.es / 16);
      s.moved += 2 * cnt * k.es;
    }
  }
  size_t off = 0, cnt = 0;
  zc_chunk(k.count, k.es, N, me, &off, &cnt);
  FoldStep& f = p.k[1];
  f.nseg = cnt > 0 ? 1 : 0;
  f.seg[0].src_off = f.seg[0].dst_off = off * k.es;
  f.seg[0].count = cnt * k.es;
  f.seg[0].src_mask = 1u << me;
  f.seg[0].dst_mask = everyone(N) & ~(1u << me) & ~(1u << k.root);
  f.packets = cnt * k.es / 16;
  f.moved = (size_t)(N - 1) * cnt * k.es;
  return p;
}

// Push-only (XMPI_ALGO_ZPUSH): the fold with nothing READ over xGMI -- loads over a link are round trips, stores are posted.
// Two device-synchronised kernels: every rank stores its contribution to chunk q into region `me` of rank q's own block
// (DsyncCall::own_block: the communicator's staging area, announced with the buffers; chunks cut as the fold cuts them, zc_chunk
// -- so in place and ragged counts work like anything else); then, all of chunk `me` being local, folds it in rank order and
// stores the result into its place in everybody's receive buffer.  One hop each way, S / N per link direction and kernel.
FoldPlan plan_push_only(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  size_t maxc = 0;
  for (int q = 0; q < N; q++) {
    size_t off = 0, cnt = 0;
    zc_chunk(k.count, k.es, N, q, &off, &cnt);
    maxc = std::max(maxc, cnt * k.es);
  }
  const size_t region = (maxc + 255) / 256 * 256;
  FoldPlan p;
  p.kernels = 2;
  p.land = region * (size_t)N;
  FoldStep& s = p.k[0];
  for (int q = 0; q < N; q++) {
    size_t off = 0, cnt = 0;
    zc_chunk(k.count, k.es, N, q, &off, &cnt);
    if (q == me || cnt == 0) continue;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = off * k.es;           // my contribution to chunk q ...
    g.dst_off = (size_t)me * region;  // ... into region `me` of rank q's block
    g.count = cnt * k.es;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << q;
    g.dst_to_land = 1;
    s.packets = std::max(s.packets, cnt * k.es / 16);
    s.moved += 2 * cnt * k.es;
  }
  // every contribution to chunk `me` is local now (the first kernel's close: every peer's stores have landed): ONE more kernel
  // folds them in rank order and stores the result into its place in everybody's receive buffer -- the fold's own kernels
  // (one kernel, or meet / body / done by size) with local sources.  Its rendezvous doubles as "my buffers may be written";
  // nobody's block is written again before its owner's next collective has announced it.
  p.k[1] = plan_fold(c, k, -1).k[0];
  p.k[1].seg[0].src_from_recv = 2;
  p.k[1].seg[0].stage_stride = region;
  return p;
}

// ring / recursive halving + doubling / binary tree: ONE kernel per rank runs every step of the schedule, the steps released by
// flag words between the peers' kernels (sched.hip) -- the schedules north_star names, without a host between their steps.
// The kernel's arguments and shape (channels, *gx workers per channel, pieces, orders: part of the signature); returns the
// traffic figure.
size_t plan_sched(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt, const DsyncArgs& a, DsyncSchedArgs* out, int* gx_out) {
  const int N = c->size, me = c->rank, coll = k.coll;
  const size_t send_bytes = k.send_bytes;
  const bool push = rt.sched_push;
  DsyncSchedArgs& sa = *out;
  memset(&sa, 0, sizeof sa);
  sa.d = a;
  sa.root = k.root;
  sa.count = k.count;
  sa.elem_size = (uint32_t)k.es;
  sa.pieces = 1;
  sa.push = push ? 1u : 0u;
  size_t step_bytes = send_bytes, traffic = 0;  // what the largest step of the schedule moves
  int nchan = 1;
  if (rt.sched_algo == XMPI_ALGO_RING) {
    sa.sched = coll == COLL_ALLREDUCE ? SCHED_RING_ALLREDUCE : SCHED_RING_ALLGATHER;
    step_bytes = coll == COLL_ALLREDUCE ? (send_bytes + (size_t)N - 1) / (size_t)N : send_bytes;
    // every channel is a different cyclic order of the ranks (plan.cpp ring_order: on an even mesh N-2 directed rings
    // that share no link direction); ranks sharing a GPU have no links to spread over
    const int avail = std::min(ring_channel_count(N), kMaxSchedChannels);
    // (the shape of a stepped kernel -- channels, workers -- is protocol: worker w waits for worker w of its peer.  It follows
    // the job's most crowded GPU, which every rank reads alike, not this rank's own: 5 ranks on 2 GPUs sit 3 + 2)
    nchan = c->sched_channels > 0 ? (int)std::min<long>(c->sched_channels, avail) : (c->dsync_sharers_job > 1 ? 1 : avail);
    // (reduce-scatter 2 reads + 1 write per step, allgather 1 + 1; the push form reads its own first chunk once more)
    traffic = coll == COLL_ALLREDUCE ? (5 * (size_t)(N - 1) + (push ? 1 : 0)) * step_bytes : 2 * (size_t)N * send_bytes;
  } else if (rt.sched_algo == XMPI_ALGO_RHD) {
    sa.sched = SCHED_RHD_ALLREDUCE;
    step_bytes = send_bytes / 2;
    // halving: 3 x (S/2 + S/4 + ...), doubling: 2 x the same; push form: the landing regions are written and read -- one more
    traffic = (push ? 6 : 5) * (send_bytes - send_bytes / (size_t)N);
    if ((N & (N - 1)) != 0) traffic += 3 * send_bytes;     // (no power of two: the fold-in / fold-out steps, at most)
  } else {
    sa.sched = coll == COLL_BCAST ? SCHED_TREE_BCAST : SCHED_TREE_REDUCE;
    const size_t piece = (size_t)std::max<long>(4096, c->tree_piece_bytes);
    sa.pieces = (int)std::min<size_t>(32, std::max<size_t>(1, (send_bytes + piece - 1) / piece));
    step_bytes = (send_bytes + (size_t)sa.pieces - 1) / (size_t)sa.pieces;
    const int v = (me - k.root + N) % N;
    const size_t children = (size_t)((2 * v + 1 < N) + (2 * v + 2 < N));
    if (coll == COLL_BCAST) {  // pull: a node reads its parent's piece and writes its own; push: it reads its own and writes each child's
      traffic = push ? 2 * send_bytes * children : (me == k.root ? 0 : 2 * send_bytes);
    } else {  // pull: 2 reads + 1 write per child; push: own input + one slot per child read, one buffer stored (upwards, or the result)
      traffic = push ? (children + 2) * send_bytes : 3 * send_bytes * children;
    }
  }
  const size_t tiles = std::max<size_t>(1, (step_bytes + kSchedTileBytes - 1) / kSchedTileBytes);
  const long job_cap = c->dsync_grid_cap > 0 ? c->dsync_grid_cap : 1024 / std::max(1, c->dsync_sharers_job);
  long workers = c->sched_grid > 0 ? c->sched_grid : (long)std::min<size_t>(tiles, (size_t)job_cap);
  workers = std::max<long>(1, std::min<long>(workers, kStepSlots));
  nchan = (int)std::max<long>(1, std::min<long>(nchan, workers));
  const int gx = (int)std::max<long>(1, workers / nchan);
  sa.nchan = nchan;
  // (worker w of a rank waits for worker w of its peer, over the same channels and pieces: the shape is part of the call)
  sa.d.sig = sig_fold(sig_mix(sig_mix(sig_mix(a.sig, (uint64_t)nchan), (uint64_t)gx), (uint64_t)sa.pieces));
  for (int ch = 0; ch < nchan; ch++) {
    std::vector<int> ord;
    ring_order(N, ch, &ord);
    for (int i = 0; i < N; i++) sa.order[ch][i] = (uint8_t)ord[(size_t)i];
  }
  *gx_out = gx;
  return traffic;
}

// one rendezvous + data movement + completion exchange: ONE kernel, or -- large messages -- meet / body / done.  A blocking call
// learns that the collective is over from a word its closing block writes (dsync_status bytes 16..23), not from an event: set on
// the LAST kernel of the collective only -- and not at all when a copy-out kernel behind it writes the word (host_out)
int launch_fold(DsyncCall& call, DsyncArgs& a, const FoldStep& s, int unroll, bool last) {
  xmpi_comm* const c = call.c;
  ++c->dsync_epoch;  // the host's count (the kernels count for themselves, from the page: see epoch_floor)
  if (!call.prof_events()) return XMPI_ERR_HIP;
  memcpy(a.seg, s.seg, sizeof a.seg);
  a.nseg = s.nseg;
  a.host_done = last && !call.host_out ? call.done_dev : nullptr;
  a.done_value = call.done_id;
  const bool split = a.nseg > 0 && c->dsync_res &&
                     (s.split_pref >= 0 ? s.split_pref != 0 : (c->dsync_split_bytes > 0 && s.moved >= (size_t)c->dsync_split_bytes));
  RoctxRange lr("xmpi:launch %s nsrc=%d bytes=%zu epoch=%llu", split ? (c->body_sys ? "meet/body(sys)/done" : "meet/body/done") : "fold",
                s.nsrc, s.moved, (unsigned long long)c->dsync_epoch);
  if (split) {
    XMPI_HIP(launch_dsync_meet(a, c->dsync_res, call.stream));
    XMPI_HIP(launch_dsync_body(c->dsync_res, a.nseg, s.packets + 1, s.nsrc, s.dtype, s.op, s.moved, c->body_sys != 0, call.stream,
                               call.pstart, call.pstop));
    XMPI_HIP(launch_dsync_done(a, c->dsync_res, call.stream));
    c->dsync_launches += 3;
    c->dsync_split_launches++;
    return XMPI_OK;
  }
  const int gx = a.nseg > 0 ? dsync_grid(c, s.packets, a.nseg, unroll) : 1;
  XMPI_HIP(launch_dsync_fold(a, s.nsrc, s.dtype, s.op, gx, unroll, call.stream, call.pstart, call.pstop));
  c->dsync_launches++;
  return XMPI_OK;
}

int launch_sched(DsyncCall& call, DsyncSchedArgs& sa, int gx, int dtype, int op) {
  xmpi_comm* const c = call.c;
  ++c->dsync_epoch;
  if (!call.prof_events()) return XMPI_ERR_HIP;
  sa.d.host_done = call.host_out ? nullptr : call.done_dev;
  sa.d.done_value = call.done_id;
  RoctxRange lr("xmpi:launch sched=%d channels=%d workers=%d pieces=%d epoch=%llu", sa.sched, sa.nchan, gx, sa.pieces,
                (unsigned long long)c->dsync_epoch);
  XMPI_HIP(launch_dsync_sched(sa, dtype, op, gx, call.stream, call.pstart, call.pstop));
  c->dsync_launches++;
  c->dsync_sched_launches++;
  return XMPI_OK;
}

// Buffers the peers can map.  Anything else -- host memory, device memory that was never registered -- is stood in for by a block
// of a registered arena (one local copy in, one out); the collective itself is the same zero-copy exchange.  Also where the result
// of a stand-in goes home from, and how.  A failure is the call's (DsyncCall::fail), but under capture, which lends nothing.
int resolve_buffers(DsyncCall& call, const CollArgs& k, const DsyncRoute& rt, const void* sendbuf, void* recvbuf, bool capturing, Resolved* r) {
  xmpi_comm* const c = call.c;
  const int N = c->size, me = c->rank, coll = k.coll;
  const bool recv_significant = coll != COLL_REDUCE || me == k.root;
  const bool in_place = sendbuf == recvbuf;
  // a capture bakes addresses into the graph: a stand-in would be given back to the arena while replays still use it
  auto no_standin = [] {
    set_last_error("graph capture needs registered device buffers (xmpi_malloc / xmpi_register)");
    return XMPI_ERR_ARG;
  };
  int rc = XMPI_OK;
  r->send = sendbuf;
  r->recv = recv_significant ? recvbuf : const_cast<void*>(sendbuf);
  if (!zc_export(c, r->send, k.send_bytes, &r->sref)) {
    if (capturing) return no_standin();
    r->tmp_send = lend_standin(c, call.lent, k.send_bytes, &r->sref, &rc);
    if (!r->tmp_send) return call.fail(rc);
    if (coll != COLL_BCAST || me == k.root) {
      // a host slice of a blocking call goes in through pinned memory the GPU reads itself (memcpy + one small kernel in
      // stream order) -- the runtime's copy out of pageable memory is a staged, synchronous affair of 10 us and more
      const bool pinned = call.blocking && k.send_bytes <= xmpi_comm::kHostBounce && c->p2p_tickets && !is_device_pointer(sendbuf) &&
                          host_bounce_ready(c);
      if (pinned) memcpy(c->host_bounce, sendbuf, k.send_bytes);
      const hipError_t e = pinned ? bounce_copy(c, r->tmp_send, c->host_bounce_dev, k.send_bytes, 0, nullptr, 0, call.stream)
                                  : hipMemcpyAsync(r->tmp_send, sendbuf, k.send_bytes, hipMemcpyDefault, call.stream);
      if (e != hipSuccess) return call.fail(hip_fail(e, "copy into a stand-in", __FILE__, __LINE__));
      if (pinned) c->host_bounce_calls++;
    }
    r->send = r->tmp_send;
  }
  if (!recv_significant || (in_place && coll != COLL_ALLGATHER)) {
    r->recv = const_cast<void*>(r->send);
    r->rref = r->sref;
  } else if (!zc_export(c, r->recv, k.recv_bytes, &r->rref)) {
    if (capturing) return no_standin();
    r->tmp_recv = lend_standin(c, call.lent, k.recv_bytes, &r->rref, &rc);
    if (!r->tmp_recv) return call.fail(rc);
    r->recv = r->tmp_recv;
  }
  // binary-tree reduce, pull form: an inner node that is not the root accumulates its subtree's partial result in a block the
  // parent can read (sched_steps.h SCHED_TREE_REDUCE); the caller's receive buffer means nothing there.  (Never under capture:
  // the route runs a captured tree reduce as the fold.)
  if (rt.form == DsyncRoute::STEPPED && !rt.sched_push && coll == COLL_REDUCE && me != k.root && 2 * ((me - k.root + N) % N) + 1 < N) {
    r->recv = call.own_block(k.send_bytes);
    if (!r->recv) return call.fail(XMPI_ERR_NOMEM);
    if (!zc_export(c, r->recv, k.send_bytes, &r->rref)) return call.fail(XMPI_ERR_HIP);
  }
  // where the result of a stand-in goes home from, and how: a host slice of a blocking call comes out through pinned memory --
  // one more small kernel in stream order copies the stand-in there and THEN writes the completion word
  call.out_src = r->tmp_recv ? r->tmp_recv
                 : (r->tmp_send && recv_significant && (in_place || coll == COLL_BCAST) && coll != COLL_ALLGATHER) ? r->tmp_send
                                                                                                                   : nullptr;
  call.host_out = call.blocking && call.out_src && k.recv_bytes <= xmpi_comm::kHostBounce && c->p2p_tickets && c->dsync_status_dev &&
                  !is_device_pointer(recvbuf) && host_bounce_ready(c);
  return XMPI_OK;
}

// the peers know the allocations: both buffers are published, and every peer has mapped them
int announce(xmpi_comm* c, const Resolved& r, bool capturing, int* sslot, int* rslot) {
  uint64_t ps = 0, pr = 0;
  int rc = publish(c, r.sref, sslot, &ps, capturing);
  if (rc == XMPI_OK) rc = publish(c, r.rref, rslot, &pr, capturing);
  if (rc == XMPI_OK) rc = await_acks(c, std::max(ps, pr));
  return rc;
}

// ... and the communicator's landing block (DsyncCall::own_block) a push form's peers store into: into d's land_* fields
int announce_land(DsyncCall& call, size_t bytes, bool capturing, DsyncArgs* d) {
  void* const own = call.own_block(bytes);
  if (!own) return XMPI_ERR_NOMEM;
  BufRef lref;
  if (!zc_export(call.c, own, bytes, &lref)) return XMPI_ERR_HIP;
  int slot = 0;
  uint64_t pi = 0;
  int rc = publish(call.c, lref, &slot, &pi, capturing);
  if (rc == XMPI_OK) rc = await_acks(call.c, pi);
  if (rc != XMPI_OK) return rc;
  d->land_gen = lref.gen;
  d->land_off = lref.offset;
  d->land_slot = (uint64_t)slot;
  d->my_land = own;
  return XMPI_OK;
}

// what every kernel of the collective is told: the pages, this rank's announced buffers, where it reports
DsyncArgs meet_args(const xmpi_comm* c, const Resolved& r, int sslot, int rslot) {
  DsyncArgs a;
  memset(&a, 0, sizeof a);
  for (int p = 0; p < c->size; p++) a.page[p] = c->peer_page[p];
  a.me = c->rank;
  a.n = c->size;
  a.send_gen = r.sref.gen;
  a.send_off = r.sref.offset;
  a.send_slot = (uint64_t)sslot;
  a.recv_gen = r.rref.gen;
  a.recv_off = r.rref.offset;
  a.recv_slot = (uint64_t)rslot;
  a.table = c->dsync_table_dev;
  a.tag = c->dsync_tag;
  a.epoch_floor = c->dsync_base;
  a.host_epoch = c->dsync_status_dev ? (uint64_t*)(c->dsync_status_dev + 2) : nullptr;
  a.my_send = r.send;
  a.my_recv = r.recv;
  a.abort_word = c->dsync_abort_dev;
  a.status = c->dsync_status_dev;
  a.xcc_need = (c->xcd_check && !c->body_sys) ? c->xcds : 0;  // (body_sys: the data kernel needs no L2 to have been acquired)
  a.spin_limit = c->timeout_s > 0 ? (uint64_t)c->timeout_s * 100000000ull : 0;  // wall_clock64 ticks at 100 MHz
  return a;
}

}  // namespace

// One device-synchronised collective, enqueued on `stream`.  blocking: wait for it (the xmpi_allreduce family);
// otherwise return once it is enqueued (xmpi_*_on_stream).  Every rank of the job takes this path for the same
// calls (the decision depends on the communicator and the arguments only), so the epochs agree.
int dsync_collective(xmpi_comm* c, int coll, int root, const void* sendbuf, void* recvbuf, size_t count, int dtype,
                     int op, hipStream_t stream, bool blocking, int algo) {
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype);
  const CollArgs k{coll, root, dtype, op, count, es, count * es, coll_send_bytes(coll, c->size, count * es), coll_recv_bytes(coll, c->size, count * es)};
  if (!stream) stream = c->local_stream;
  DsyncCall call(c, stream, blocking);
  dsync_service(c);
  reap_deferred(c, false);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream, &cap);
  (void)hipGetLastError();
  const bool capturing = cap != hipStreamCaptureStatusNone;

  // route: a refused call and an LL call end here
  const DsyncRoute rt = dsync_route(c, coll, algo, k.unit, capturing);
  if (rt.refused >= 0) return refuse(coll, rt.refused);
  if (rt.form == DsyncRoute::LL) return dsync_ll(call, k, sendbuf, recvbuf, capturing);
  RoctxRange range("xmpi:dsync %s algo=%s bytes=%zu epoch=%llu %s", coll_name(coll), algo_name(rt.algo), k.send_bytes,
                   (unsigned long long)c->dsync_epoch + 1, blocking ? "blocking" : capturing ? "captured" : "enqueued");

  // resolve the buffers, announce them
  Resolved r;
  int rc = resolve_buffers(call, k, rt, sendbuf, recvbuf, capturing, &r);
  if (rc != XMPI_OK) return rc;
  int sslot = 0, rslot = 0;
  rc = announce(c, r, capturing, &sslot, &rslot);
  if (rc == XMPI_OK) rc = order_behind_last(c, stream, capturing);
  if (rc != XMPI_OK) return call.fail(rc);

  // build and launch the kernel(s)
  call.begin(capturing);
  DsyncArgs a = meet_args(c, r, sslot, rslot);
  a.sig = call_sig(c, k, rt);
  if (rt.form == DsyncRoute::STEPPED) {
    DsyncSchedArgs sa;
    int gx = 1;
    call.traffic = plan_sched(c, k, rt, a, &sa, &gx);
    // push form: the block the peers store into where this rank's receive buffer cannot take their data yet (sched_steps.h
    // sched_land_bytes: in-place ring allreduce -- the receive buffer still is the input; halving -- a region per level; tree
    // reduce -- a slot per child).  (Never under capture: the route runs a captured push form as its pull form.)
    const size_t land = (size_t)sched_land_bytes(sa, r.send == r.recv);
    c->dsync_land_bytes = land;
    if (land) rc = announce_land(call, land, capturing, &sa.d);
    if (rc == XMPI_OK) rc = launch_sched(call, sa, gx, dtype, op);
  } else {
    const FoldPlan p = rt.form == DsyncRoute::PUSH_ONLY        ? (coll == COLL_REDUCE_SCATTER ? plan_reduce_scatter_push(c, k) : plan_push_only(c, k))
                       : coll == COLL_REDUCE_SCATTER           ? plan_reduce_scatter(c, k, rt.split_pref)
                       : coll == COLL_ALLTOALL                 ? plan_alltoall(c, k, rt.split_pref)
                       : coll == COLL_ALLGATHER                ? plan_allgather(c, k, rt.split_pref)
                       : coll != COLL_BCAST                    ? plan_fold(c, k, rt.split_pref)
                       : bcast_forwards(c, k.send_bytes)       ? plan_bcast_forward(c, k)
                                                               : plan_bcast_push(c, k);
    if (p.land) {
      rc = announce_land(call, p.land, capturing, &a);
      if (rc == XMPI_OK) c->dsync_land_bytes = p.land;
    }
    for (int i = 0; rc == XMPI_OK && i < p.kernels; i++) {
      call.traffic += p.k[i].moved;
      rc = launch_fold(call, a, p.k[i], rt.unroll, i + 1 == p.kernels);
    }
  }
  if (rc != XMPI_OK) return call.fail(rc);
  if (!capturing) c->dsync_last_stream = stream;
  if (call.host_out) {
    const hipError_t e = bounce_copy(c, c->host_bounce_dev + xmpi_comm::kHostBounce, call.out_src, k.recv_bytes, 1, call.done_dev,
                                     call.done_id, stream);
    if (e != hipSuccess) return call.fail(hip_fail(e, "copy of a stand-in's result into pinned memory", __FILE__, __LINE__));
    c->host_bounce_calls++;
  }

  // finish
  return blocking ? call.wait_and_finish(recvbuf, k.recv_bytes) : call.enqueued(recvbuf, k.recv_bytes);
}

// ---- xmpi_alltoallv: every pair its own count, read and exchanged by the kernel ---------------------------------------------------
// What the reference's own program does (helloworld.go:53-81: messages of different lengths, and Receive re-sizes the destination to
// whatever arrived, network.go:594-601) as ONE kernel per rank (kernels.hip dsync_alltoallv_kernel).  The host knows the two EXTENTS
// only: it announces them like any collective's buffers and sizes the grid from the send extent; counts and displacements are read
// by the kernel when it runs -- from the caller's device arrays (stream form: a captured launch replays with whatever they hold
// then), or from the communicator's pinned record a blocking call fills.
// Only meet-on-the-device, one kernel: the split (meet / body / done) form and an LL-line form do not exist for it.
namespace {
enum { VREC_SENDCOUNTS = 0, VREC_SDISPLS = 1, VREC_RECVCAPS = 2, VREC_RDISPLS = 3, VREC_RECVCOUNTS = 4, VREC_ARRAYS = 5 };

// a buffer of the call the peers can map: the caller's, or -- host memory, unregistered device memory, nothing at all (an extent
// of 0) -- a registered stand-in of the extent's size, lent into `lent`
void* v_mappable(xmpi_comm* c, std::vector<void*>& lent, const void* p, size_t bytes, BufRef* ref, bool* stood_in, int* rc) {
  *stood_in = false;
  if (bytes > 0 && zc_export(c, p, bytes, ref)) return const_cast<void*>(p);
  *stood_in = true;
  return lend_standin(c, lent, std::max<size_t>(bytes, 16), ref, rc);
}
}  // namespace

int dsync_alltoallv(xmpi_comm* c, const void* sendbuf, size_t send_extent, void* recvbuf, size_t recv_extent, const VArrays& v, int dtype,
                    hipStream_t stream, bool blocking) {
  const int N = c->size;
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype), sb = send_extent * es, rb = recv_extent * es;
  if (!stream) stream = c->local_stream;
  DsyncCall call(c, stream, blocking);
  dsync_service(c);
  reap_deferred(c, false);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream, &cap);
  (void)hipGetLastError();
  const bool capturing = cap != hipStreamCaptureStatusNone;
  RoctxRange range("xmpi:dsync alltoallv send_extent=%zu recv_extent=%zu epoch=%llu %s", sb, rb, (unsigned long long)c->dsync_epoch + 1,
                   blocking ? "blocking" : capturing ? "captured" : "enqueued");

  // the arrays the kernel reads: the caller's (stream form), or the pinned record
  VArrays dv = v;
  if (blocking) {
    if (!c->v_rec) pinned_words(sizeof(uint64_t) * VREC_ARRAYS * kDsyncRanks, &c->v_rec, &c->v_rec_dev);
    if (!c->v_rec || !c->v_rec_dev) {
      set_last_error("alltoallv: no pinned memory for the record of counts");
      return XMPI_ERR_NOMEM;
    }
    const uint64_t* in[4] = {v.sendcounts, v.sdispls, v.recvcaps, v.rdispls};
    for (int k = 0; k < 4; k++) memcpy(c->v_rec + k * kDsyncRanks, in[k], sizeof(uint64_t) * (size_t)N);
    memset(c->v_rec + VREC_RECVCOUNTS * kDsyncRanks, 0, sizeof(uint64_t) * kDsyncRanks);
    dv.sendcounts = c->v_rec_dev + VREC_SENDCOUNTS * kDsyncRanks;
    dv.sdispls = c->v_rec_dev + VREC_SDISPLS * kDsyncRanks;
    dv.recvcaps = c->v_rec_dev + VREC_RECVCAPS * kDsyncRanks;
    dv.rdispls = c->v_rec_dev + VREC_RDISPLS * kDsyncRanks;
    dv.recvcounts = c->v_rec_dev + VREC_RECVCOUNTS * kDsyncRanks;
  }

  // the buffers: stand-ins of the extents' size for what the peers cannot map.  A blocking call keeps its receive stand-in past
  // the wait (`keep`) and copies down the delivered blocks alone; an enqueued one, which has no counts, loads the stand-in from the
  // receive buffer first and copies it back whole (DsyncCall::enqueued), so what lies between the blocks survives.
  std::vector<void*> keep;
  auto give_back = [&keep](int rc) {
    for (void* p : keep) (void)heap_free(p);
    keep.clear();
    return rc;
  };
  Resolved r;
  int rc = XMPI_OK;
  bool s_in = false, r_in = false;
  // (probe without lending: a capture must fail before anything is borrowed)
  if (capturing) {
    BufRef probe;
    if (!sb || !rb) {
      set_last_error("graph capture: an extent of 0 is stood in for by a block lent for the call, which a graph cannot hold (pass a registered "
                     "buffer of at least one element)");
      return XMPI_ERR_ARG;
    }
    if (!zc_export(c, sendbuf, sb, &probe) || !zc_export(c, recvbuf, rb, &probe)) {
      set_last_error("graph capture needs registered device buffers (xmpi_malloc / xmpi_register)");
      return XMPI_ERR_ARG;
    }
  }
  r.send = v_mappable(c, call.lent, sendbuf, sb, &r.sref, &s_in, &rc);
  if (!r.send) return call.fail(rc);
  if (s_in && sb) {
    const hipError_t e = hipMemcpyAsync(const_cast<void*>(r.send), sendbuf, sb, hipMemcpyDefault, stream);
    if (e != hipSuccess) return call.fail(hip_fail(e, "copy into a stand-in", __FILE__, __LINE__));
  }
  r.recv = v_mappable(c, blocking ? keep : call.lent, recvbuf, rb, &r.rref, &r_in, &rc);
  if (!r.recv) return give_back(call.fail(rc));
  if (r_in && rb && !blocking) {
    const hipError_t e = hipMemcpyAsync(r.recv, recvbuf, rb, hipMemcpyDefault, stream);
    if (e != hipSuccess) return call.fail(hip_fail(e, "copy into a stand-in", __FILE__, __LINE__));
    call.out_src = r.recv;
  }
  int sslot = 0, rslot = 0;
  rc = announce(c, r, capturing, &sslot, &rslot);
  if (rc == XMPI_OK) rc = order_behind_last(c, stream, capturing);
  if (rc != XMPI_OK) return give_back(call.fail(rc));

  call.begin(capturing);
  DsyncVArgs va;
  memset(&va, 0, sizeof va);
  va.d = meet_args(c, r, sslot, rslot);
  // (the collective and the element size: the counts are nobody's to compare before the kernels have exchanged them)
  va.d.sig = sig_fold(sig_mix(sig_mix(0x9E3779B97F4A7C15ull, (uint64_t)COLL_COUNT + 1), (uint64_t)es));
  va.d.host_done = call.done_dev;
  va.d.done_value = call.done_id;
  va.sendcounts = dv.sendcounts;
  va.sdispls = dv.sdispls;
  va.recvcaps = dv.recvcaps;
  va.rdispls = dv.rdispls;
  va.recvcounts = dv.recvcounts;
  va.send_extent = send_extent;
  va.recv_extent = recv_extent;
  va.vstatus = c->dsync_status_dev ? c->dsync_status_dev + 13 : nullptr;
  if (!call.prof_events()) return give_back(call.fail(XMPI_ERR_HIP));
  ++c->dsync_epoch;
  {
    // the host may not know the counts: the grid follows the send extent (every block strides over whatever tiles there are)
    const int gx = dsync_grid(c, sb / 16, 1, 4);
    const hipError_t le = launch_dsync_alltoallv(va, (int)es, gx, stream, call.pstart, call.pstop);
    if (le != hipSuccess) {
      --c->dsync_epoch;
      return give_back(call.fail(hip_fail(le, "alltoallv kernel launch", __FILE__, __LINE__)));
    }
  }
  c->dsync_launches++;
  c->dsync_v_launches++;
  if (!capturing) c->dsync_last_stream = stream;
  call.traffic = 2 * sb;
  if (!blocking) return call.enqueued(recvbuf, rb);

  rc = call.wait_and_finish(nullptr, 0);
  if (rc != XMPI_OK && rc != XMPI_ERR_TRUNCATE && rc != XMPI_ERR_ARG) return give_back(rc);
  const uint64_t* got = c->v_rec + VREC_RECVCOUNTS * kDsyncRanks;
  memcpy(v.recvcounts, got, sizeof(uint64_t) * (size_t)N);
  if (r_in) {  // the delivered blocks go home: rows that held, counts that fitted
    hipError_t e = hipSuccess;
    for (int p = 0; p < N && e == hipSuccess; p++) {
      const bool row_ok = v.sdispls[p] <= send_extent && v.sendcounts[p] <= send_extent - v.sdispls[p] && v.rdispls[p] <= recv_extent &&
                          v.recvcaps[p] <= recv_extent - v.rdispls[p];
      if (!row_ok || got[p] == 0 || got[p] > v.recvcaps[p]) continue;
      e = hipMemcpyAsync((char*)recvbuf + v.rdispls[p] * es, (const char*)r.recv + v.rdispls[p] * es, got[p] * es, hipMemcpyDefault, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return give_back(hip_fail(e, "copy of a stand-in's delivered blocks", __FILE__, __LINE__));
  }
  return give_back(rc);
}

// ---- stream-ordered Send / Receive ------------------------------------------------------------------------------------
// The reference's Send is a gob message on a net.Conn and a wait for the ack message (network.go:562-571), its Receive
// reads, routes by tag, acks and decodes (network.go:575-625).  Here both are ONE kernel each, enqueued on a stream:
// the sender's writes {message number, tag, dtype, bytes, where the payload lives} into a box of the receiver's flag
// allocation (64 bytes over xGMI) and waits for the answer; the receiver's waits for a box with its tag, pulls the
// payload straight out of the sender's HBM and answers.  Nothing is polled by a host thread.  (The blocking
// xmpi_send / xmpi_recv do NOT use waiting kernels -- p2p.cpp: a kernel that waits for a peer holds its hardware
// queue, and the reference's semantics let a program block in several Sends / Receives at once, in any order.)

namespace {

int p2p_done_slot(xmpi_comm* c, uint64_t* id_out) {
  const uint64_t id = ++c->p2p_done_next;
  *id_out = id;
  const int slot = (int)(id % xmpi_comm::kP2PDoneSlots);
  __atomic_store_n(&c->p2p_done[4 * slot], 0, __ATOMIC_RELEASE);
  return slot;
}

int p2p_status_to_rc(uint64_t st) {
  if (st == 0) return XMPI_OK;
  if (st >= 0x100) {
    const uint32_t why = (uint32_t)(st - 0x100);
    if (why == DSYNC_TIMEOUT) {
      set_last_error("send / receive: the peer did not arrive within XMPI_TIMEOUT_S (kernel wait cut short)");
      return XMPI_ERR_TIMEOUT;
    }
    if (why == DSYNC_UNMAPPED) {
      set_last_error("receive: the sender's buffer is not mapped here");
      return XMPI_ERR_STATE;
    }
    set_last_error("send / receive: the job was aborted while the kernel waited");  // (callers with the communicator at hand say why: abort_reason)
    return XMPI_ERR_PEER;
  }
  if (st == 6) set_last_error("receive: the message does not fit the buffer");
  else set_last_error("receive: dtype differs from the sender's");
  return -(int)st;
}

void p2p_fill(xmpi_comm* c, P2PArgs* a, int peer, int tag, int dtype) {
  memset(a, 0, sizeof *a);
  a->my_page = c->dpage;
  a->peer_page = c->peer_page[peer];
  a->me = c->rank;
  a->peer = peer;
  a->tag = tag;
  a->dtype = dtype;
  a->comm_tag = c->dsync_tag;
  a->table = c->dsync_table_dev;
  a->abort_word = c->dsync_abort_dev;
  a->spin_limit = c->timeout_s > 0 ? (uint64_t)c->timeout_s * 100000000ull : 0;
}

}  // namespace

// the operations that have completed since the last look: their stand-ins go back, the first failure is returned
int dsync_p2p_reap(xmpi_comm* c) {
  int rc = XMPI_OK;
  for (size_t i = 0; i < c->p2p_pending.size();) {
    xmpi_comm::P2PPending& p = c->p2p_pending[i];
    if (__atomic_load_n(&c->p2p_done[4 * p.slot], __ATOMIC_ACQUIRE) != p.id) {
      i++;
      continue;
    }
    const int r = p2p_status_to_rc(c->p2p_done[4 * p.slot + 1]);
    if (r != XMPI_OK && rc == XMPI_OK) rc = r;
    for (void* b : p.bufs) (void)heap_free(b);
    c->p2p_pending.erase(c->p2p_pending.begin() + (long)i);
  }
  return rc;
}

int dsync_send(xmpi_comm* c, const void* buf, size_t bytes, int dtype, int dest, int tag, hipStream_t stream) {
  RoctxRange range("xmpi:send_on_stream dest=%d tag=%d bytes=%zu", dest, tag, bytes);
  if (!stream) stream = c->local_stream;
  dsync_service(c);
  if ((int)c->p2p_pending.size() >= xmpi_comm::kP2PDoneSlots - 2) {  // completion words are a ring: do not lap it
    set_last_error("too many stream-ordered sends / receives outstanding: xmpi_stream_sync first");
    return XMPI_ERR_STATE;
  }
  BufRef ref;
  memset(&ref, 0, sizeof ref);
  std::vector<void*> lent;
  int slot = 0;
  if (bytes > 0) {
    int rc = XMPI_OK;
    if (!zc_export(c, buf, bytes, &ref)) {  // memory the receiver cannot map: a registered stand-in (one local copy)
      void* tmp = lend_standin(c, lent, bytes, &ref, &rc);
      const hipError_t e = tmp ? hipMemcpyAsync(tmp, buf, bytes, hipMemcpyDeviceToDevice, stream) : hipSuccess;
      if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync(stand-in)", __FILE__, __LINE__);
    }
    uint64_t pi = 0;
    if (rc == XMPI_OK) rc = publish(c, ref, &slot, &pi);
    if (rc == XMPI_OK) rc = await_acks(c, pi);
    if (rc != XMPI_OK) {
      for (void* p : lent) (void)heap_free(p);
      return rc;
    }
  }
  P2PArgs a;
  p2p_fill(c, &a, dest, tag, dtype);
  a.seq = ((c->dsync_tag & 0xffffffffull) << 32) | (c->p2p_out_seq[dest] + 1);  // (consumed below, once the kernel is enqueued)
  a.bytes = bytes;
  a.gen = ref.gen;
  a.slot = (uint64_t)slot;
  a.off = ref.offset;
  uint64_t id = 0;
  const int ds = p2p_done_slot(c, &id);
  a.host_done = c->p2p_done_dev + 4 * ds;
  a.done_value = id;
  if (launch_p2p_send(a, stream) != hipSuccess) {
    // message n was never posted: its number must not be consumed (message n + 8 would wait for its ack for ever)
    const int rc = hip_fail(hipGetLastError(), "p2p send kernel", __FILE__, __LINE__);
    for (void* p : lent) (void)heap_free(p);
    return rc;
  }
  ++c->p2p_out_seq[dest];
  c->p2p_pending.push_back({ds, id, lent});
  return XMPI_OK;
}

int dsync_recv(xmpi_comm* c, void* buf, size_t cap_bytes, int dtype, int src, int tag, hipStream_t stream) {
  RoctxRange range("xmpi:recv_on_stream src=%d tag=%d capacity=%zu", src, tag, cap_bytes);
  if (!stream) stream = c->local_stream;
  dsync_service(c);
  if ((int)c->p2p_pending.size() >= xmpi_comm::kP2PDoneSlots - 2) {
    set_last_error("too many stream-ordered sends / receives outstanding: xmpi_stream_sync first");
    return XMPI_ERR_STATE;
  }
  P2PArgs a;
  p2p_fill(c, &a, src, tag, dtype);
  a.bytes = cap_bytes;
  a.buf = buf;
  // unique per PAGE, not per communicator: the page is pooled and never cleared, a later communicator's first receive must
  // not match the go record an earlier one left behind (the communicator number is what a.seq carries as well)
  a.op_id = ((c->dsync_tag & 0xffffffffull) << 32) | (++c->p2p_op_id & 0xffffffffull);
  uint64_t id = 0;
  const int ds = p2p_done_slot(c, &id);
  a.host_done = c->p2p_done_dev + 4 * ds;
  a.done_value = id;
  // a few blocks for a large message; every block but the first only waits for the first (a local word)
  long gx = (long)((cap_bytes + 16383) >> 14);
  gx = std::max<long>(1, std::min<long>(gx, c->dsync_sharers > 1 ? 16 : 128));
  XMPI_HIP(launch_p2p_recv(a, (int)gx, stream));
  c->p2p_pending.push_back({ds, id, {}});
  return XMPI_OK;
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
