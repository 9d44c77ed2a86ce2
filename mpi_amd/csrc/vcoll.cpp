// vcoll.cpp -- xmpi_alltoallv: the public entry points, and the form for ranks that meet on the host.
//
// What the reference's own program performs (helloworld.go:53-81) is an all-to-all in which every pair has its own count and the
// receiver learns it from the message (network.go:594-601).  With ranks that meet on the device the counts are read and exchanged
// by the kernel itself (dsync.cpp dsync_alltoallv).  Ranks that meet on the host -- rank threads of one process, XMPI_DSYNC=0, more
// than kDsyncRanks ranks, XMPI_ZERO_COPY=0, or DIRECT by name -- take the form below: the {count, capacity} pairs through the
// equal-count xmpi_alltoall, then the blocks over the blocking Send / Receive in N rounds of disjoint pairs.  The same results and
// the same errors; correct rather than fast.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "comm.h"
#include "kernels.h"
#include "trace.h"

namespace xmpi {

// round `round` of N: the partner of rank `me` -- a perfect matching of the ranks (a rank may be its own partner), and over the N
// rounds every rank meets every rank, itself included, exactly once
int v_round_partner(int round, int me, int n) { return ((round - me) % n + n) % n; }

namespace {

constexpr uint64_t kValidBit = 1ull << 63;  // of the capacity word: the row it comes from held

struct VCall {
  const void* sendbuf;
  size_t send_extent;
  const uint64_t *sendcounts, *sdispls;
  void* recvbuf;
  size_t recv_extent;
  const uint64_t *recvcaps, *rdispls;
  uint64_t* recvcounts;
  int dtype;
  size_t es;
};

bool row_ok(const VCall& q, int j) {
  return q.sdispls[j] <= q.send_extent && q.sendcounts[j] <= q.send_extent - q.sdispls[j] && q.rdispls[j] <= q.recv_extent &&
         q.recvcaps[j] <= q.recv_extent - q.rdispls[j];
}

// what both forms check before anything moves, from the arguments alone
int v_check_args(const xmpi_comm* c, const VCall& q) {
  if (q.es == 0 || !q.sendcounts || !q.sdispls || !q.recvcaps || !q.rdispls || !q.recvcounts) {
    set_last_error("alltoallv: bad dtype / null array");
    return XMPI_ERR_ARG;
  }
  if ((q.send_extent && !q.sendbuf) || (q.recv_extent && !q.recvbuf)) {
    set_last_error("alltoallv: null buffer");
    return XMPI_ERR_ARG;
  }
  if (q.send_extent > SIZE_MAX / 16 || q.recv_extent > SIZE_MAX / 16) {
    set_last_error("alltoallv: extent out of range");
    return XMPI_ERR_ARG;
  }
  const uintptr_t s = (uintptr_t)q.sendbuf, r = (uintptr_t)q.recvbuf;
  if (q.send_extent && q.recv_extent && s < r + q.recv_extent * q.es && r < s + q.send_extent * q.es) {
    set_last_error("alltoallv is out of place only: the send and the receive buffer overlap");
    return XMPI_ERR_ARG;
  }
  (void)c;
  return XMPI_OK;
}

// memory a kernel can read and write: device memory, or host memory that is pinned / registered (pageable host memory is neither)
bool device_addressable(const void* p) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeHost;
}

bool v_on_device(const xmpi_comm* c, int algo) {
  if (!dsync_usable(c) || c->size > kDsyncRanks || algo == XMPI_ALGO_DIRECT) return false;
  return algo == XMPI_ALGO_ZCOPY || !c->windows_ok || c->zero_copy != 0;
}

int v_local_copy(xmpi_comm* c, void* dst, const void* src, size_t bytes) {
  XMPI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->local_stream));
  XMPI_HIP(hipStreamSynchronize(c->local_stream));
  return XMPI_OK;
}

int v_on_host(xmpi_comm* c, const VCall& q) {
  const int N = c->size, me = c->rank;
  std::vector<uint64_t> out(2 * (size_t)N), in(2 * (size_t)N);
  int bad = -1, trunc = -1;
  for (int j = 0; j < N; j++) {
    const bool ok = row_ok(q, j);
    out[2 * (size_t)j] = ok ? q.sendcounts[j] : 0;
    out[2 * (size_t)j + 1] = ok ? (q.recvcaps[j] | kValidBit) : 0;
    if (!ok && bad < 0) bad = j;
  }
  if (N > 1) {
    const int rc = xmpi_alltoall(c, out.data(), in.data(), 2, XMPI_I64, XMPI_ALGO_AUTO);
    if (rc != XMPI_OK) return rc;
  } else {
    in = out;
  }
  for (int r = 0; r < N; r++) q.recvcounts[r] = in[2 * (size_t)r];
  for (int round = 0; round < N; round++) {
    const int p = v_round_partner(round, me, N);
    const uint64_t send_n = out[2 * (size_t)p], my_cap = out[2 * (size_t)p + 1] & ~kValidBit;
    const uint64_t recv_n = in[2 * (size_t)p], peer_cap = in[2 * (size_t)p + 1] & ~kValidBit;
    const bool pair = (out[2 * (size_t)p + 1] & kValidBit) && (in[2 * (size_t)p + 1] & kValidBit);
    if (!pair) continue;
    if ((send_n > peer_cap || recv_n > my_cap) && (trunc < 0 || p < trunc)) trunc = p;
    const bool do_send = send_n > 0 && send_n <= peer_cap, do_recv = recv_n > 0 && recv_n <= my_cap;
    const char* from = (const char*)q.sendbuf + q.sdispls[p] * q.es;
    char* to = (char*)q.recvbuf + q.rdispls[p] * q.es;
    int rc = XMPI_OK;
    if (p == me) {
      if (do_send) rc = v_local_copy(c, to, from, send_n * q.es);
    } else {
      size_t got = 0;
      for (int half = 0; half < 2 && rc == XMPI_OK; half++) {  // the lower rank sends first
        const bool sends = (half == 0) == (me < p);
        if (sends && do_send) rc = p2p_send(c, from, send_n * q.es, q.dtype, p, kVTag);
        if (!sends && do_recv) rc = p2p_recv(c, to, recv_n * q.es, q.dtype, p, kVTag, &got);
      }
    }
    if (rc != XMPI_OK) return rc;
  }
  if (bad >= 0) {
    set_last_error("alltoallv: the arrays' row for rank " + std::to_string(bad) + " leaves the extents of the buffers; nothing was moved between the two");
    return XMPI_ERR_ARG;
  }
  if (trunc >= 0) {
    set_last_error("alltoallv: the block exchanged with rank " + std::to_string(trunc) + " is longer than the capacity its receiver granted; it was not moved");
    return XMPI_ERR_TRUNCATE;
  }
  return XMPI_OK;
}

}  // namespace
}  // namespace xmpi

using namespace xmpi;

extern "C" {

int xmpi_alltoallv_partner(int round, int rank, int size) { return (size > 0 && rank >= 0 && rank < size) ? v_round_partner(round, rank, size) : -1; }

int xmpi_alltoallv(xmpi_comm* c, const void* sendbuf, size_t send_extent, const uint64_t* sendcounts, const uint64_t* sdispls, void* recvbuf,
                   size_t recv_extent, const uint64_t* recvcaps, const uint64_t* rdispls, uint64_t* recvcounts, xmpi_dtype dtype, int algo) {
  XMPI_ENTER(c);
  if (algo != XMPI_ALGO_AUTO && algo != XMPI_ALGO_ZCOPY && algo != XMPI_ALGO_DIRECT) {
    set_last_error(std::string("alltoallv has no ") + (algo >= 0 && algo < XMPI_ALGO_COUNT ? algo_name(algo) : "such") + " schedule (zcopy | direct | auto)");
    return XMPI_ERR_UNSUPPORTED;
  }
  const VCall q{sendbuf, send_extent, sendcounts, sdispls, recvbuf, recv_extent, recvcaps, rdispls, recvcounts, (int)dtype, xmpi_dtype_size(dtype)};
  const int rc = v_check_args(c, q);
  if (rc != XMPI_OK) return rc;
  drain_worker(c);
  if (v_on_device(c, algo)) {
    std::lock_guard<std::mutex> g(c->coll_mu);
    const VArrays v{sendcounts, sdispls, recvcaps, rdispls, recvcounts};
    return dsync_alltoallv(c, sendbuf, send_extent, recvbuf, recv_extent, v, (int)dtype, c->local_stream, /*blocking=*/true);
  }
  return v_on_host(c, q);
}

int xmpi_alltoallv_on_stream(xmpi_comm* c, const void* sendbuf, size_t send_extent, const uint64_t* sendcounts, const uint64_t* sdispls,
                             void* recvbuf, size_t recv_extent, const uint64_t* recvcaps, const uint64_t* rdispls, uint64_t* recvcounts,
                             xmpi_dtype dtype, void* stream) {
  XMPI_ENTER(c);
  const VCall q{sendbuf, send_extent, sendcounts, sdispls, recvbuf, recv_extent, recvcaps, rdispls, recvcounts, (int)dtype, xmpi_dtype_size(dtype)};
  const int rc = v_check_args(c, q);
  if (rc != XMPI_OK) return rc;
  if (!dsync_usable(c) || c->size > kDsyncRanks) {
    set_last_error("stream-ordered alltoallv needs ranks that meet on the device (one process per GPU): the counts are read by the kernel");
    return XMPI_ERR_UNSUPPORTED;
  }
  if ((send_extent && !is_device_pointer(sendbuf)) || (recv_extent && !is_device_pointer(recvbuf))) {
    set_last_error("stream-ordered collectives take device memory (use the blocking forms for host buffers)");
    return XMPI_ERR_ARG;
  }
  for (const void* arr : {(const void*)sendcounts, (const void*)sdispls, (const void*)recvcaps, (const void*)rdispls, (const void*)recvcounts})
    if (!device_addressable(arr)) {
      set_last_error("stream-ordered alltoallv: the five arrays are read and written by the kernel -- device memory or pinned host memory "
                     "(host arrays: the blocking form)");
      return XMPI_ERR_ARG;
    }
  drain_worker(c);
  std::lock_guard<std::mutex> g(c->coll_mu);
  const VArrays v{sendcounts, sdispls, recvcaps, rdispls, recvcounts};
  return dsync_alltoallv(c, sendbuf, send_extent, recvbuf, recv_extent, v, (int)dtype, stream ? (hipStream_t)stream : c->local_stream,
                         /*blocking=*/false);
}

}  // extern "C"
