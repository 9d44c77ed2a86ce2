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
// This file is one collective, start to end (dsync_collective; its LL form, dsync_ll).  Its siblings, sharing dsync.h:
//   dsync_plan.cpp   what a call is and what every rank launches for it -- route, signature, segments, grid; pure
//   dsync_call.cpp   the call lifecycle (DsyncCall): publish / acks, lent blocks, the pinned bounce, waits, profile harvest, dsync_check
//   dsync_p2p.cpp    stream-ordered Send / Receive
//   vcoll.cpp        xmpi_alltoallv, whose device form is built from the same parts
//   dsync_conn.cpp   the connection lifecycle (dsync_prepare / dsync_connect / the helper thread / dsync_finalize) and dsync_service
#include <algorithm>
#include <cstring>

#include "dsync.h"
#include "sched_steps.h"

namespace xmpi {

static_assert(kDsyncRanks <= kMaxRanks, "the device side serves a subset of the jobs the host side admits");

// ---- LL small collectives (ll.hip): the payload is pushed into the peers' flag allocations, nothing is registered,
// announced or translated; one kernel, one one-way hop.  Whether a call goes this way is decided by dsync_collective from the
// arguments and the job's layout only (the same on every rank); what kind of memory a rank passes is this rank's business.
static int dsync_ll(DsyncCall& call, const CollArgs& k, const void* sendbuf, void* recvbuf) {
  const bool capturing = call.capturing;
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
  // (the agent knows the four collectives whose ranks all send the same line; reduce-scatter and all-to-all are launched -- and so is
  // a REDUCTION of an 8-bit float type: the agent's kernel is not taught the two types, which keeps its registers as they were, and
  // its command names a dtype in three bits)
  const bool f8_fold = dtype_is_f8(k.dtype) && (coll == COLL_ALLREDUCE || coll == COLL_REDUCE);
  if (blocking && !capturing && !coll_personal(coll) && !f8_fold && call.lent.empty() && c->agent_ll && unit <= agent_limit && !c->prof_on &&
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
  const int rc = call.order_behind_last();
  if (rc != XMPI_OK) return call.fail(rc);
  call.begin();

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
  a.spin_limit = spin_limit_ticks(c);
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

namespace {

int dsync_refuse(int coll, int cand) {
  set_last_error(std::string(coll_name(coll)) + " by " + xmpi_comm::kCandName[cand] + ": refused -- it gave wrong answers on this machine when "
                 "the library checked it (xmpi_get_param \"tune_rejected_" + std::to_string(coll) + "\"; xmpi_degraded() says where)");
  return XMPI_ERR_UNSUPPORTED;
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
int resolve_buffers(DsyncCall& call, const CollArgs& k, const DsyncRoute& rt, const void* sendbuf, void* recvbuf, Resolved* r) {
  xmpi_comm* const c = call.c;
  const int N = c->size, me = c->rank, coll = k.coll;
  const bool recv_significant = coll != COLL_REDUCE || me == k.root;
  const bool in_place = sendbuf == recvbuf;
  int rc = XMPI_OK;
  r->send = sendbuf;
  r->recv = recv_significant ? recvbuf : const_cast<void*>(sendbuf);
  if (!zc_export(c, r->send, k.send_bytes, &r->sref)) {
    if (call.capturing) return capture_needs_registered();
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
    if (call.capturing) return capture_needs_registered();
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

}  // namespace

// the peers know the allocations: both buffers are published, and every peer has mapped them
int dsync_announce(DsyncCall& call, const Resolved& r, int* sslot, int* rslot) {
  xmpi_comm* const c = call.c;
  uint64_t ps = 0, pr = 0;
  int rc = dsync_publish(c, r.sref, sslot, &ps, call.capturing);
  if (rc == XMPI_OK) rc = dsync_publish(c, r.rref, rslot, &pr, call.capturing);
  if (rc == XMPI_OK) rc = dsync_await_acks(c, std::max(ps, pr));
  return rc;
}

// ... and the communicator's landing block (DsyncCall::own_block) a push form's peers store into: into d's land_* fields
static int announce_land(DsyncCall& call, size_t bytes, DsyncArgs* d) {
  void* const own = call.own_block(bytes);
  if (!own) return XMPI_ERR_NOMEM;
  BufRef lref;
  if (!zc_export(call.c, own, bytes, &lref)) return XMPI_ERR_HIP;
  int slot = 0;
  uint64_t pi = 0;
  int rc = dsync_publish(call.c, lref, &slot, &pi, call.capturing);
  if (rc == XMPI_OK) rc = dsync_await_acks(call.c, pi);
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
  a.spin_limit = spin_limit_ticks(c);
  return a;
}

// One device-synchronised collective, enqueued on `stream`.  blocking: wait for it (the xmpi_allreduce family);
// otherwise return once it is enqueued (xmpi_*_on_stream).  Every rank of the job takes this path for the same
// calls (the decision depends on the communicator and the arguments only), so the epochs agree.
int dsync_collective(xmpi_comm* c, int coll, int root, const void* sendbuf, void* recvbuf, size_t count, int dtype,
                     int op, hipStream_t stream, bool blocking, int algo) {
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype);
  const CollArgs k{coll, root, dtype, op, count, es, count * es, coll_send_bytes(coll, c->size, count * es), coll_recv_bytes(coll, c->size, count * es)};
  DsyncCall call(c, stream, blocking);
  const bool capturing = call.capturing;

  // route: a refused call and an LL call end here
  const DsyncRoute rt = dsync_route(c, coll, algo, k.unit, capturing, fold_only(dtype, op) && coll_reduces(coll));
  if (rt.refused >= 0) return dsync_refuse(coll, rt.refused);
  if (rt.form == DsyncRoute::LL) return dsync_ll(call, k, sendbuf, recvbuf);
  RoctxRange range("xmpi:dsync %s algo=%s bytes=%zu epoch=%llu %s", coll_name(coll), algo_name(rt.algo), k.send_bytes,
                   (unsigned long long)c->dsync_epoch + 1, blocking ? "blocking" : capturing ? "captured" : "enqueued");

  // resolve the buffers, announce them
  Resolved r;
  int rc = resolve_buffers(call, k, rt, sendbuf, recvbuf, &r);
  if (rc != XMPI_OK) return rc;
  int sslot = 0, rslot = 0;
  rc = dsync_announce(call, r, &sslot, &rslot);
  if (rc == XMPI_OK) rc = call.order_behind_last();
  if (rc != XMPI_OK) return call.fail(rc);

  // build and launch the kernel(s)
  call.begin();
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
    if (land) rc = announce_land(call, land, &sa.d);
    if (rc == XMPI_OK) rc = launch_sched(call, sa, gx, dtype, op);
  } else {
    const FoldPlan p = plan_for(c, k, rt);
    if (p.land) {
      rc = announce_land(call, p.land, &a);
      if (rc == XMPI_OK) c->dsync_land_bytes = p.land;
    }
    for (int i = 0; rc == XMPI_OK && i < p.kernels; i++) {
      call.traffic += p.k[i].moved;
      rc = launch_fold(call, a, p.k[i], rt.unroll, i + 1 == p.kernels);
    }
  }
  if (rc != XMPI_OK) return call.fail(rc);
  if (!capturing) c->dsync_last_stream = call.stream;
  if (call.host_out) {
    const hipError_t e = bounce_copy(c, c->host_bounce_dev + xmpi_comm::kHostBounce, call.out_src, k.recv_bytes, 1, call.done_dev,
                                     call.done_id, call.stream);
    if (e != hipSuccess) return call.fail(hip_fail(e, "copy of a stand-in's result into pinned memory", __FILE__, __LINE__));
    c->host_bounce_calls++;
  }

  // finish
  return blocking ? call.wait_and_finish(recvbuf, k.recv_bytes) : call.enqueued(recvbuf, k.recv_bytes);
}

}  // namespace xmpi
