// ctl_selftest.cpp -- xmpi_ctl_selftest: the control plane (ctl.h) exercised by plain OS processes.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "comm.h"

using namespace xmpi;

extern "C" {

// Host-only exercise of the control plane (no HIP call): join, barriers, a token passed round the
// ring through the pipe counters and a mail-entry handshake with the next rank.  Lets the N > 1
// bootstrap / rendezvous logic be tested with plain OS processes on a machine without a GPU.
int xmpi_ctl_selftest(const char* job_key, int rank, int size, int rounds) {
  CtlConfig cfg{2, 8, 8u << 20, 2, 4u << 20, 1};  // (host lanes requested)
  std::string err;
  Ctl* ctl = nullptr;
  int rc = Ctl::join(job_key ? job_key : "selftest", rank, size, cfg, (double)env_long("XMPI_INIT_TIMEOUT_S", 30), &ctl, &err);
  if (rc != XMPI_OK) {
    set_last_error("ctl selftest: " + err);
    return rc;
  }
  auto wait_for = [&](auto pred) {
    const double t0 = now_seconds();
    Backoff bo;
    while (!pred()) {
      if (ctl->aborted()) return XMPI_ERR_PEER;
      if (now_seconds() - t0 > 30.0) return XMPI_ERR_TIMEOUT;
      bo.pause();
    }
    return XMPI_OK;
  };
  const int next = (rank + 1) % size, prev = (rank + size - 1) % size;
  for (int k = 1; k <= rounds && rc == XMPI_OK; k++) {
    rc = ctl->barrier(30.0);
    if (rc != XMPI_OK || size == 1) continue;
    // token round the ring through the head counters
    if (rank == 0) {
      ctl->pipe(0, next, 0)->head.v.store((uint64_t)k, std::memory_order_release);
      rc = wait_for([&] { return ctl->pipe(prev, 0, 0)->head.v.load(std::memory_order_acquire) == (uint64_t)k; });
    } else {
      rc = wait_for([&] { return ctl->pipe(prev, rank, 0)->head.v.load(std::memory_order_acquire) == (uint64_t)k; });
      ctl->pipe(rank, next, 0)->head.v.store((uint64_t)k, std::memory_order_release);
    }
    if (rc != XMPI_OK) break;
    // tagged rendezvous with the next rank (the states of a Send / Receive pair, without payload)
    MailEntry* out = ctl->mail(rank, next, k % kMailEntries);
    uint32_t expect = MAIL_FREE;
    if (!out->state.compare_exchange_strong(expect, MAIL_CLAIMED)) {
      rc = XMPI_ERR_STATE;
      break;
    }
    out->tag = k;
    out->bytes = (uint64_t)k * 10u + (uint64_t)rank;
    memset(&out->src, 0, sizeof out->src);  // the direct-pull offer of a registered payload travels with the header
    out->src.base = 0x1000u * (uint64_t)(rank + 1);
    out->src.gen = (uint64_t)k;
    out->src.offset = (uint64_t)rank;
    out->direct.store(DIRECT_OFFERED, std::memory_order_relaxed);
    out->state.store(MAIL_POSTED, std::memory_order_release);
    MailEntry* in = ctl->mail(prev, rank, k % kMailEntries);
    rc = wait_for([&] { return in->state.load(std::memory_order_acquire) == MAIL_POSTED && in->tag == k; });
    if (rc != XMPI_OK) break;
    if (in->bytes != (uint64_t)k * 10u + (uint64_t)prev || in->direct.load(std::memory_order_acquire) != DIRECT_OFFERED ||
        in->src.base != 0x1000u * (uint64_t)(prev + 1) || in->src.gen != (uint64_t)k || in->src.offset != (uint64_t)prev) {
      rc = XMPI_ERR_STATE;
      break;
    }
    in->direct.store(k % 2 ? DIRECT_ACCEPTED : DIRECT_DECLINED, std::memory_order_release);
    in->state.store(MAIL_DONE, std::memory_order_release);
    rc = wait_for([&] { return out->state.load(std::memory_order_acquire) == MAIL_DONE; });
    if (rc == XMPI_OK && out->direct.load(std::memory_order_acquire) != (k % 2 ? DIRECT_ACCEPTED : DIRECT_DECLINED))
      rc = XMPI_ERR_STATE;
    out->state.store(MAIL_FREE, std::memory_order_release);
    if (rc != XMPI_OK) break;
    // a host-resident payload through the entry's host lane (p2p.cpp send_through_host_lane / recv_from_host_lane, DIRECT_HOST): a ring of
    // kHostLaneSlots pieces, head written by the sender, tail by the receiver; every rank sends to the next and receives from
    // the one before at once, lengths from one byte to three times the ring
    if (ctl->host_lane_bytes() > 0) {
      const size_t lane_bytes = ctl->host_lane_bytes(), piece = lane_bytes / kHostLaneSlots;
      auto length = [&](int r) { return (size_t)(((uint64_t)k * 7919u + (uint64_t)r * 104729u) % (3u * lane_bytes)) + 1; };
      auto byte_at = [&](int r, size_t i) { return (uint8_t)(i * 31u + (size_t)k + (size_t)r * 7u); };
      const int e = k % kMailEntries;
      const size_t out_bytes = length(rank), in_bytes = length(prev);
      const uint64_t out_np = (out_bytes + piece - 1) / piece, in_np = (in_bytes + piece - 1) / piece;
      char* lane_out = ctl->host_lane(rank, next, e);
      const char* lane_in = ctl->host_lane(prev, rank, e);
      PipeCtl* po = &ctl->mail(rank, next, e)->pipe;
      PipeCtl* pin = &ctl->mail(prev, rank, e)->pipe;
      std::vector<uint8_t> got(in_bytes);
      uint64_t filled = 0, taken = 0;
      const double t0 = now_seconds();
      Backoff bo;
      while ((filled < out_np || taken < in_np) && rc == XMPI_OK) {
        bool moved = false;
        if (filled < out_np && filled - po->tail.v.load(std::memory_order_acquire) < (uint64_t)kHostLaneSlots) {
          const size_t off = (size_t)filled * piece, n = std::min(piece, out_bytes - off);
          char* slot = lane_out + (size_t)(filled % kHostLaneSlots) * piece;
          for (size_t i = 0; i < n; i++) slot[i] = (char)byte_at(rank, off + i);
          po->head.v.store(++filled, std::memory_order_release);
          moved = true;
        }
        if (taken < in_np && pin->head.v.load(std::memory_order_acquire) > taken) {
          const size_t off = (size_t)taken * piece, n = std::min(piece, in_bytes - off);
          memcpy(got.data() + off, lane_in + (size_t)(taken % kHostLaneSlots) * piece, n);
          pin->tail.v.store(++taken, std::memory_order_release);
          moved = true;
        }
        if (!moved) {
          if (ctl->aborted()) rc = XMPI_ERR_PEER;
          else if (now_seconds() - t0 > 30.0) rc = XMPI_ERR_TIMEOUT;
          bo.pause();
        }
      }
      for (size_t i = 0; i < in_bytes && rc == XMPI_OK; i++)
        if (got[i] != byte_at(prev, i)) {
          set_last_error("ctl selftest: host lane payload differs at byte " + std::to_string(i) + " of " + std::to_string(in_bytes));
          rc = XMPI_ERR_STATE;
        }
      if (rc != XMPI_OK) break;
      rc = ctl->barrier(30.0);  // everybody has drained its lane: the counters start the next message at zero
      if (rc != XMPI_OK) break;
      po->head.v.store(0, std::memory_order_relaxed);
      pin->tail.v.store(0, std::memory_order_relaxed);
      rc = ctl->barrier(30.0);
      if (rc != XMPI_OK) break;
    }
    // zero-copy collective k: descriptors are double-buffered by sequence parity; everybody reads
    // everybody's after the barrier, a rank that freed buffers says so in its retire log
    BufDesc* mine = ctl->desc(rank, (uint64_t)k);
    mine->ok = 1;
    mine->fresh = (k + rank) % 3 == 0;
    mine->send.base = 0x100000u * (uint64_t)(rank + 1) + (uint64_t)k;
    mine->send.gen = (uint64_t)k * 100u + (uint64_t)rank;
    mine->recv = mine->send;
    mine->recv.offset = 64u * (uint64_t)k;
    for (size_t b = 0; b < sizeof mine->send.handle; b++) mine->send.handle[b] = (uint8_t)(b + (size_t)rank + (size_t)k);
    mine->seq.store((uint64_t)k, std::memory_order_release);
    RetireLog* log = ctl->retired(rank);
    for (int j = 0; j < rank + 1; j++) {  // rank r retires r+1 allocations per round
      const uint64_t n = log->count.load(std::memory_order_relaxed);
      log->gen[n % kRetireRing] = ((uint64_t)rank << 32) | n;
      log->count.store(n + 1, std::memory_order_release);
    }
    rc = ctl->barrier(30.0);
    if (rc != XMPI_OK) break;
    for (int p = 0; p < size && rc == XMPI_OK; p++) {
      const BufDesc* d = ctl->desc(p, (uint64_t)k);
      const RetireLog* lp = ctl->retired(p);
      const uint64_t n = lp->count.load(std::memory_order_acquire);
      bool good = d->seq.load(std::memory_order_acquire) == (uint64_t)k && d->ok == 1 && d->fresh == ((k + p) % 3 == 0) &&
                  d->send.base == 0x100000u * (uint64_t)(p + 1) + (uint64_t)k &&
                  d->send.gen == (uint64_t)k * 100u + (uint64_t)p && d->recv.offset == 64u * (uint64_t)k &&
                  d->send.handle[5] == (uint8_t)(5 + p + k) && n == (uint64_t)k * (uint64_t)(p + 1);
      for (uint64_t j = n > (uint64_t)kRetireRing ? n - kRetireRing : 0; j < n && good; j++)
        good = lp->gen[j % kRetireRing] == (((uint64_t)p << 32) | j);
      if (!good) rc = XMPI_ERR_STATE;
    }
    if (rc != XMPI_OK) break;
    // device-synchronised collectives: a rank publishes a registration (slot k % 4), every peer reads it and
    // acknowledges, and the owner goes on only when all have (dsync_call.cpp `dsync_publish` / `dsync_await_acks`, dsync_conn.cpp `dsync_service`)
    PubTable* pt = ctl->published(rank);
    const uint64_t n = pt->count.load(std::memory_order_relaxed);
    PubEntry& pe = pt->e[n % kPubRing];
    pe.gen = (uint64_t)k * 1000u + (uint64_t)rank;
    pe.base = 0x200000u * (uint64_t)(rank + 1);
    pe.bytes = (uint64_t)k << 20;
    pe.reserved = (uint64_t)(k % 4);
    for (size_t b = 0; b < sizeof pe.handle; b++) pe.handle[b] = (uint8_t)(b ^ (size_t)rank ^ (size_t)k);
    pt->count.store(n + 1, std::memory_order_release);
    bool mine_acked = false;
    std::vector<uint64_t> seen((size_t)size, (uint64_t)(k - 1));
    rc = wait_for([&] {
      for (int p = 0; p < size; p++) {  // serve the peers while waiting for them, like every wait loop of the library
        if (p == rank) continue;
        PubTable* pp = ctl->published(p);
        const uint64_t np = pp->count.load(std::memory_order_acquire);
        while (seen[(size_t)p] < np) {
          const PubEntry& e = pp->e[seen[(size_t)p] % kPubRing];
          const uint64_t kk = seen[(size_t)p] + 1;  // entry number == round it was published in
          if (e.gen != kk * 1000u + (uint64_t)p || e.base != 0x200000u * (uint64_t)(p + 1) || e.bytes != (kk << 20) ||
              e.reserved != kk % 4 || e.handle[7] != (uint8_t)(7 ^ (size_t)p ^ (size_t)kk))
            return true;  // corrupt entry: leave the wait, the check below fails
          seen[(size_t)p]++;
        }
        ctl->acked(rank, p)->store(seen[(size_t)p], std::memory_order_release);
      }
      mine_acked = true;
      bool served_all = true;  // (the library keeps serving from inside its barrier; here: stay until every peer's entry of this round is acknowledged)
      for (int p = 0; p < size; p++) {
        if (p == rank) continue;
        if (ctl->acked(p, rank)->load(std::memory_order_acquire) < n + 1) mine_acked = false;
        if (seen[(size_t)p] < n + 1) served_all = false;
      }
      return mine_acked && served_all;
    });
    if (rc == XMPI_OK && !mine_acked) rc = XMPI_ERR_STATE;
    if (rc != XMPI_OK) break;
    rc = ctl->barrier(30.0);  // nobody starts the next round's publication before everybody has checked this one
  }
  if (rc != XMPI_OK) ctl->set_abort(rc);
  else rc = ctl->barrier(30.0);
  delete ctl;
  return rc;
}

}  // extern "C"
