// dsync_p2p.cpp -- stream-ordered Send / Receive (xmpi_send_on_stream / xmpi_recv_on_stream) between ranks that meet on the device.
//
// The reference's Send is a gob message on a net.Conn and a wait for the ack message (network.go:562-571), its Receive
// reads, routes by tag, acks and decodes (network.go:575-625).  Here both are ONE kernel each, enqueued on a stream:
// the sender's writes {message number, tag, dtype, bytes, where the payload lives} into a box of the receiver's flag
// allocation (64 bytes over xGMI) and waits for the answer; the receiver's waits for a box with its tag, pulls the
// payload straight out of the sender's HBM and answers.  Nothing is polled by a host thread.  (The blocking
// xmpi_send / xmpi_recv do NOT use waiting kernels -- p2p.cpp: a kernel that waits for a peer holds its hardware
// queue, and the reference's semantics let a program block in several Sends / Receives at once, in any order.)
#include <cstring>

#include "dsync.h"

namespace xmpi {

namespace {

// the next completion word of the ring, cleared, and where the operation's kernel reports into it
int p2p_done_slot(xmpi_comm* c, P2PArgs* a) {
  const uint64_t id = ++c->p2p_done_next;
  const int slot = (int)(id % xmpi_comm::kP2PDoneSlots);
  __atomic_store_n(&c->p2p_done[4 * slot], 0, __ATOMIC_RELEASE);
  a->host_done = c->p2p_done_dev + 4 * slot;
  a->done_value = id;
  return slot;
}

// completion words are a ring: do not lap it
int p2p_ring_has_room(const xmpi_comm* c) {
  if ((int)c->p2p_pending.size() < xmpi_comm::kP2PDoneSlots - 2) return XMPI_OK;
  set_last_error("too many stream-ordered sends / receives outstanding: xmpi_stream_sync first");
  return XMPI_ERR_STATE;
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
  a->spin_limit = spin_limit_ticks(c);
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
  if (const int full = p2p_ring_has_room(c)) return full;
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
    if (rc == XMPI_OK) rc = dsync_publish(c, ref, &slot, &pi);
    if (rc == XMPI_OK) rc = dsync_await_acks(c, pi);
    if (rc != XMPI_OK) {
      for (void* p : lent) (void)heap_free(p);
      return rc;
    }
  }
  P2PArgs a;
  p2p_fill(c, &a, dest, tag, dtype);
  a.seq = c->p2p_out_seq[dest] + 1;  // all 64 bits, and nothing else in the word (consumed below, once the kernel is enqueued)
  a.bytes = bytes;
  a.gen = ref.gen;
  a.slot = (uint64_t)slot;
  a.off = ref.offset;
  const int ds = p2p_done_slot(c, &a);
  if (launch_p2p_send(a, stream) != hipSuccess) {
    // message n was never posted: its number must not be consumed (message n + 8 would wait for its ack for ever)
    const int rc = hip_fail(hipGetLastError(), "p2p send kernel", __FILE__, __LINE__);
    for (void* p : lent) (void)heap_free(p);
    return rc;
  }
  ++c->p2p_out_seq[dest];
  c->p2p_pending.push_back({ds, a.done_value, lent});
  return XMPI_OK;
}

int dsync_recv(xmpi_comm* c, void* buf, size_t cap_bytes, int dtype, int src, int tag, hipStream_t stream) {
  RoctxRange range("xmpi:recv_on_stream src=%d tag=%d capacity=%zu", src, tag, cap_bytes);
  if (!stream) stream = c->local_stream;
  dsync_service(c);
  if (const int full = p2p_ring_has_room(c)) return full;
  P2PArgs a;
  p2p_fill(c, &a, src, tag, dtype);
  a.bytes = cap_bytes;
  a.buf = buf;
  // unique per communicator, never 0: the go records of the (pooled) page were cleared when this communicator connected
  a.op_id = ++c->p2p_op_id;
  const int ds = p2p_done_slot(c, &a);
  // a few blocks for a large message; every block but the first only waits for the first (a local word)
  long gx = (long)((cap_bytes + 16383) >> 14);
  gx = std::max<long>(1, std::min<long>(gx, c->dsync_sharers > 1 ? 16 : 128));
  if (c->p2p_grid_cap > 0) gx = std::min<long>(gx, c->p2p_grid_cap);  // ("p2p_grid_cap" / XMPI_P2P_GRID_CAP, as the blocking Receive's pull kernel)
  XMPI_HIP(launch_p2p_recv(a, (int)gx, stream));
  c->p2p_pending.push_back({ds, a.done_value, {}});
  return XMPI_OK;
}

}  // namespace xmpi
