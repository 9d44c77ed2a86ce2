// vcoll.cpp -- xmpi_alltoallv whole: the public entry points and both forms, for ranks that meet on the host and on the device.
//
// What the reference's own program performs (helloworld.go:53-81) is an all-to-all in which every pair has its own count and the
// receiver learns it from the message (network.go:594-601).  With ranks that meet on the device the counts are read and exchanged
// by the kernel itself (dsync_alltoallv below, on the parts dsync.h shares).  Ranks that meet on the host -- rank threads of one
// process, XMPI_DSYNC=0, more than kDsyncRanks ranks, XMPI_ZERO_COPY=0, or DIRECT by name -- take v_on_host: the {count, capacity}
// pairs through the equal-count xmpi_alltoall, then the blocks over the blocking Send / Receive in N rounds of disjoint pairs.  The
// same results and the same errors; correct rather than fast.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "dsync.h"
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

// ---- the form for ranks that meet on the device: every pair its own count, read and exchanged by the kernel -------------------------
// What the reference's own program does (helloworld.go:53-81: messages of different lengths, and Receive re-sizes the destination to
// whatever arrived, network.go:594-601) as ONE kernel per rank (kernels.hip dsync_alltoallv_kernel).  The host knows the two EXTENTS
// only: it announces them like any collective's buffers and sizes the grid from the send extent; counts and displacements are read
// by the kernel when it runs -- from the caller's device arrays (stream form: a captured launch replays with whatever they hold
// then), or from the communicator's pinned record a blocking call fills.
// Only meet-on-the-device, one kernel: the split (meet / body / done) form and an LL-line form do not exist for it.
enum { VREC_SENDCOUNTS = 0, VREC_SDISPLS = 1, VREC_RECVCAPS = 2, VREC_RDISPLS = 3, VREC_RECVCOUNTS = 4, VREC_ARRAYS = 5 };

// a buffer of the call the peers can map: the caller's, or -- host memory, unregistered device memory, nothing at all (an extent
// of 0) -- a registered stand-in of the extent's size, lent into `lent`
void* v_mappable(xmpi_comm* c, std::vector<void*>& lent, const void* p, size_t bytes, BufRef* ref, bool* stood_in, int* rc) {
  *stood_in = false;
  if (bytes > 0 && zc_export(c, p, bytes, ref)) return const_cast<void*>(p);
  *stood_in = true;
  return lend_standin(c, lent, std::max<size_t>(bytes, 16), ref, rc);
}

// The five arrays are memory the device addresses (`stream` form), or -- blocking, host arrays -- go through the communicator's pinned
// record.  Extents and the arrays' contents in elements.
struct VArrays {
  const uint64_t *sendcounts, *sdispls, *recvcaps, *rdispls;
  uint64_t* recvcounts;
};

int dsync_alltoallv(xmpi_comm* c, const void* sendbuf, size_t send_extent, void* recvbuf, size_t recv_extent, const VArrays& v, int dtype,
                    hipStream_t stream, bool blocking) {
  const int N = c->size;
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype), sb = send_extent * es, rb = recv_extent * es;
  DsyncCall call(c, stream, blocking);
  stream = call.stream;  // (0 was the communicator's own)
  const bool capturing = call.capturing;
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
    if (!zc_export(c, sendbuf, sb, &probe) || !zc_export(c, recvbuf, rb, &probe)) return capture_needs_registered();
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
  rc = dsync_announce(call, r, &sslot, &rslot);
  if (rc == XMPI_OK) rc = call.order_behind_last();
  if (rc != XMPI_OK) return give_back(call.fail(rc));

  call.begin();
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
