// api.cpp -- the extern "C" entry points of include/xmpi.h.  Compiled by hipcc as host code.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

static thread_local std::string g_last_error;
thread_local uint64_t t_api_call = 0;  // the number of the public call this thread is in (XMPI_ENTER)

void set_last_error(const std::string& s) { g_last_error = s; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  const char* base = strrchr(file, '/');
  g_last_error = std::string(what) + " failed: " + hipGetErrorString(e) + " (" + (base ? base + 1 : file) + ":" +
                 std::to_string(line) + ")";
  (void)hipGetLastError();
  return XMPI_ERR_HIP;
}

// XMPI_TRACE=1: one line per bootstrap step on stderr (where does a rank that hangs in Init hang?)
bool trace_on() {
  static const bool on = getenv("XMPI_TRACE") && atoi(getenv("XMPI_TRACE")) != 0;
  return on;
}

long env_long(const char* name, long dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  long x = strtol(v, &end, 0);
  return (end && end != v) ? x : dflt;
}

static size_t choose_piece(const xmpi_comm* c, size_t bytes_per_rank_chunk) {
  if (c->piece_bytes > 0) return std::min<size_t>((size_t)c->piece_bytes, c->slot_bytes);
  // ranks sharing one in-order stream have nothing to overlap: one launch per chunk
  if (c->shared_stream && all_peers_colocated(c)) return c->slot_bytes;
  // ~4 pieces per chunk so a chunk's transfer overlaps its reduction, but never below 1 MiB (a piece
  // costs a launch and an event: ~10 us, i.e. ~0.5 MiB of link time), within [1 MiB, slot]
  size_t p = 1u << 20;
  while (p * 4 < bytes_per_rank_chunk && p < c->slot_bytes) p <<= 1;
  return std::min(p, c->slot_bytes);
}

// ---- non-blocking collectives: an ordered worker per communicator --------------------------------
static thread_local bool t_in_worker = false;

static void worker_main(xmpi_comm* c) {
  t_in_worker = true;
  (void)hipSetDevice(c->device);
  for (;;) {
    std::pair<std::function<int()>, xmpi_request*> job;
    {
      std::unique_lock<std::mutex> l(c->wq_mu);
      c->wq_cv.wait(l, [c] { return c->wq_stop || !c->wq.empty(); });
      if (c->wq.empty()) return;  // stop requested and nothing left to run
      job = std::move(c->wq.front());
      c->wq.pop_front();
    }
    g_last_error.clear();
    t_api_call = c->api_calls.fetch_add(1, std::memory_order_relaxed) + 1;  // (before the job takes coll_mu: whoever holds it next has seen this -- dsync.cpp dsync_ll)
    const int rc = job.first();
    {
      std::lock_guard<std::mutex> l(job.second->mu);
      job.second->rc = rc;
      job.second->err = g_last_error;
      job.second->done = true;
      job.second->cv.notify_all();  // under the lock: the waiter frees the request as soon as it sees `done`
    }
    {
      std::lock_guard<std::mutex> l(c->wq_mu);
      c->wq_busy--;
    }
    c->wq_cv.notify_all();
  }
}

static xmpi_request* submit(xmpi_comm* c, std::function<int()> fn) {
  xmpi_request* r = new xmpi_request;
  {
    std::lock_guard<std::mutex> l(c->wq_mu);
    if (!c->worker_started) {
      c->worker = std::thread(worker_main, c);
      c->worker_started = true;
    }
    c->wq.emplace_back(std::move(fn), r);
    c->wq_busy++;
  }
  c->wq_cv.notify_all();
  return r;
}

// a blocking collective issued after non-blocking ones runs after them (same order on every rank)
void drain_worker(xmpi_comm* c) {
  if (t_in_worker || !c->worker_started) return;
  std::unique_lock<std::mutex> l(c->wq_mu);
  c->wq_cv.wait(l, [c] { return c->wq_busy == 0; });
}

void stop_worker(xmpi_comm* c) {
  if (!c->worker_started) return;
  drain_worker(c);
  {
    std::lock_guard<std::mutex> l(c->wq_mu);
    c->wq_stop = true;
  }
  c->wq_cv.notify_all();
  c->worker.join();
  c->worker_started = false;
}

// (called with c->coll_mu held; ranks that meet on the host)
static int collective_on_host_meeting_ranks(xmpi_comm* c, int coll, int algo, int root, const void* sendbuf, void* recvbuf, size_t count, int dtype,
                                            int op) {
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype);
  // Zero-copy first (zcopy.cpp): when every rank's buffers are registered HBM one kernel per rank does
  // the whole collective in place.  Whether that holds is decided collectively, so either every rank
  // returns from here or every rank goes on to the staged schedule below.
  const bool zc_algo = algo == XMPI_ALGO_ZCOPY || algo == XMPI_ALGO_ZPUSH || algo == XMPI_ALGO_LL;
  if (c->size > 1 && (zc_algo || (algo == XMPI_ALGO_AUTO && c->zero_copy))) {
    bool done = false;
    int zrc = zero_copy_collective(c, coll, root, sendbuf, recvbuf, count, dtype, op, algo == XMPI_ALGO_ZPUSH, &done);
    if (zrc != XMPI_OK || done) return zrc;
  }
  if (zc_algo) algo = XMPI_ALGO_AUTO;  // (LL lines need ranks that meet on the device: with the others it names the fold)
  // (the push forms are forms of the stepped KERNELS: the host-driven step tables have one form, which pushes into the windows)
  if (algo == XMPI_ALGO_RING_PUSH) algo = XMPI_ALGO_RING;
  if (algo == XMPI_ALGO_RHD_PUSH) algo = XMPI_ALGO_RHD;
  if (algo == XMPI_ALGO_TREE_PUSH) algo = XMPI_ALGO_TREE;
  PlanParams pp;
  pp.coll = coll;
  // (XMPI_SUM_WIDE, reduce: staged AUTO picks the TREE for short messages -- partial sums in T; the one-hop table folds at the root)
  // (the same for every operator on the 8-bit floats: fold_only)
  pp.algo = (fold_only(dtype, op) && coll == COLL_REDUCE && algo == XMPI_ALGO_AUTO) ? (int)XMPI_ALGO_DIRECT : algo;
  pp.size = c->size;
  pp.rank = c->rank;
  pp.root = root;
  pp.count = count;
  pp.elem_size = es;
  pp.channels = c->channels > 0 ? (int)c->channels : ring_channel_count(c->size);  // 0 = every link
  pp.lanes = c->lanes;
  const size_t total = count * es;
  size_t chunk = total;
  if (coll == COLL_ALLREDUCE) chunk = total / (size_t)c->size / (size_t)std::max(1, pp.channels);
  pp.piece_bytes = choose_piece(c, chunk);
  pp.fuse = 1;  // ring: receive-reduce-send / receive-copy-send as one kernel
  pp.fifo_depth = c->fifo_depth;
  pp.oneshot_bytes = (size_t)std::max<long>(0, c->oneshot_bytes);
  Plan plan;
  int rc = build_plan(pp, &plan);
  if (rc != XMPI_OK) {
    set_last_error("no schedule for this collective / algorithm / size");
    return rc;
  }

  // host-resident buffers: stage through this rank's HBM (convenience path; the hot path is HBM)
  const bool send_dev = is_device_pointer(sendbuf), recv_dev = is_device_pointer(recvbuf);
  const size_t send_bytes = coll_send_bytes(coll, c->size, total), recv_bytes = coll_recv_bytes(coll, c->size, total);
  void *dsend = const_cast<void*>(sendbuf), *drecv = recvbuf;
  void *tmp_send = nullptr, *tmp_recv = nullptr;
  if (!recv_dev) {
    XMPI_HIP(hipMalloc(&tmp_recv, recv_bytes));
    drecv = tmp_recv;
    if (coll == COLL_BCAST) XMPI_HIP(hipMemcpy(tmp_recv, recvbuf, recv_bytes, hipMemcpyHostToDevice));
  }
  if (!send_dev) {
    if (sendbuf == recvbuf && coll != COLL_ALLGATHER && !coll_personal(coll)) {
      if (coll != COLL_BCAST) XMPI_HIP(hipMemcpy(drecv, sendbuf, send_bytes, hipMemcpyHostToDevice));
      dsend = drecv;
    } else {
      XMPI_HIP(hipMalloc(&tmp_send, send_bytes));
      XMPI_HIP(hipMemcpy(tmp_send, sendbuf, send_bytes, hipMemcpyHostToDevice));
      dsend = tmp_send;
    }
  }
  rc = run_plan(c, plan, dsend, drecv, dtype, op);
  if (rc == XMPI_OK && !recv_dev) {
    const bool significant = (coll != COLL_REDUCE) || c->rank == root;
    if (significant) XMPI_HIP(hipMemcpy(recvbuf, drecv, recv_bytes, hipMemcpyDeviceToHost));
  }
  if (tmp_send) (void)hipFree(tmp_send);
  if (tmp_recv) (void)hipFree(tmp_recv);
  return rc;
}

// reduce-scatter: ZCOPY | ZPUSH | LL | DIRECT | AUTO; all-to-all: ZCOPY | LL | DIRECT | AUTO
static bool personal_algo_ok(int coll, int algo) {
  const bool ok = algo == XMPI_ALGO_AUTO || algo == XMPI_ALGO_ZCOPY || algo == XMPI_ALGO_LL || algo == XMPI_ALGO_DIRECT ||
                  (algo == XMPI_ALGO_ZPUSH && coll == COLL_REDUCE_SCATTER);
  if (!ok) set_last_error(std::string(coll_name(coll)) + " has no " + algo_name(algo) + " schedule (" +
                          (coll == COLL_REDUCE_SCATTER ? "zcopy | zpush | ll | direct | auto" : "zcopy | ll | direct | auto") + ")");
  return ok;
}

// reduce-scatter and all-to-all are out of place: a rank's receive buffer is written while peers (and its own later blocks) still
// read its send buffer
static bool personal_overlap(const xmpi_comm* c, int coll, const void* sendbuf, const void* recvbuf, size_t unit) {
  const uintptr_t s = (uintptr_t)sendbuf, r = (uintptr_t)recvbuf;
  const size_t sb = coll_send_bytes(coll, c->size, unit), rb = coll_recv_bytes(coll, c->size, unit);
  if (s >= r + rb || r >= s + sb) return false;
  set_last_error(std::string(coll_name(coll)) + " is out of place only: the send and the receive buffer overlap");
  return true;
}

static int collective(xmpi_comm* c, int coll, int algo, int root, const void* sendbuf, void* recvbuf, size_t count,
                      int dtype, int op) {
  drain_worker(c);
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype);
  if (es == 0 || op < 0 || op >= XMPI_OP_COUNT || root < 0 || root >= c->size || algo < 0 || algo >= XMPI_ALGO_COUNT) {
    set_last_error("bad dtype / op / root / algo");
    return XMPI_ERR_ARG;
  }
  if (refuse_bitwise_on_float(dtype, op)) return XMPI_ERR_ARG;  // a bitwise operator on a float type
  // XMPI_SUM_WIDE: XMPI_SUM for every type but f16 / bf16; there, a stepped schedule the caller names is refused -- its partial sums
  // travel between ranks in the 16-bit type, so no wide accumulator exists.  From the arguments alone: every rank answers alike,
  // before anything is announced or lent.
  op = normal_op(dtype, op);
  // The same for every reduction of XMPI_F8E4M3 / XMPI_F8E5M2, whatever the operator (comm.h fold_only).
  if (fold_only(dtype, op) && coll_reduces(coll) && algo_stepped(algo)) {
    if (dtype_is_f8(dtype))
      set_last_error(std::string("a reduction of XMPI_F8E4M3 / XMPI_F8E5M2 has no ") + algo_name(algo) + " schedule: ring, halving and tree pass partial results between ranks in the 8-bit type (auto | zcopy | zpush | ll | direct)");
    else
      set_last_error(std::string("XMPI_SUM_WIDE has no ") + algo_name(algo) + " schedule: ring, halving and tree pass partial sums between ranks in the 16-bit type (auto | zcopy | zpush | ll | direct)");
    return XMPI_ERR_UNSUPPORTED;
  }
  // reduce-scatter and all-to-all: the schedules that exist for them, decided from the arguments alone (every rank answers alike)
  if (coll_personal(coll) && !personal_algo_ok(coll, algo)) return XMPI_ERR_UNSUPPORTED;
  if (count == 0) return XMPI_OK;
  if (!recvbuf || !sendbuf) {
    set_last_error("null buffer");
    return XMPI_ERR_ARG;
  }
  if (coll_personal(coll) && personal_overlap(c, coll, sendbuf, recvbuf, count * es)) return XMPI_ERR_ARG;
  RoctxRange range("xmpi:%s algo=%s bytes=%zu rank=%d/%d", coll_name(coll), algo_name(algo), count * es, c->rank, c->size);
  std::lock_guard<std::mutex> g(c->coll_mu);
  // One process per GPU (the production layout): the ranks meet on the device (dsync.cpp) -- one kernel per
  // rank, enqueued on this communicator's stream, no host barrier.  Whether this path is taken depends on the
  // job's layout and the arguments only, so every rank decides alike; buffers the peers cannot map are stood in
  // for by registered arena blocks inside.
  // RING / RHD (allreduce), RING (allgather) and TREE (bcast) name the stepped kernels there (sched.hip): every step of
  // the schedule inside one kernel per rank; with ranks that meet on the host they name the staged schedules below.
  if (dsync_takes(c, coll, algo))
    return dsync_collective(c, coll, root, sendbuf, recvbuf, count, dtype, op, c->local_stream, /*blocking=*/true, algo);
  // Ranks that meet on the host, HOST slices (what a program written against the reference passes, helloworld.go:53-81): stood in
  // for by blocks of the registered arenas -- the heap keeps them from call to call, so the zero-copy fold applies and nothing is
  // hipMalloc'ed / hipFree'd per call (35 ms per 256 MiB buffer with eight rank threads at it: scripts/r06_hostleg_probe.py) --, one copy up,
  // one copy down on the communicator's stream.  No arena memory left: the staged path's own temporary buffers (below).
  const bool send_host = !is_device_pointer(sendbuf), recv_host = !is_device_pointer(recvbuf);
  if (send_host || recv_host) {
    const size_t send_bytes = coll_send_bytes(coll, c->size, count * es), recv_bytes = coll_recv_bytes(coll, c->size, count * es);
    const bool in_place = sendbuf == recvbuf && coll != COLL_ALLGATHER;
    void* up_recv = recv_host ? heap_alloc(c->device, recv_bytes) : nullptr;
    void* up_send = send_host && !(in_place && recv_host) ? heap_alloc(c->device, send_bytes) : nullptr;
    if ((recv_host && !up_recv) || (send_host && !(in_place && recv_host) && !up_send)) {
      if (up_recv) (void)heap_free(up_recv);
      if (up_send) (void)heap_free(up_send);
      (void)hipGetLastError();
      return collective_on_host_meeting_ranks(c, coll, algo, root, sendbuf, recvbuf, count, dtype, op);
    }
    void* drecv = recv_host ? up_recv : recvbuf;
    const void* dsend = !send_host ? sendbuf : (in_place && recv_host) ? drecv : up_send;
    auto done = [&](int rc) {
      if (up_recv) (void)heap_free(up_recv);
      if (up_send) (void)heap_free(up_send);
      return rc;
    };
    hipStream_t s = c->local_stream;
    // (what goes up: the operand; a broadcast's message at its root -- in `recvbuf` --; nothing else has a say in the result)
    const void* src_up = coll == COLL_BCAST ? (c->rank == root && recv_host ? recvbuf : nullptr) : (send_host ? sendbuf : nullptr);
    void* dst_up = coll == COLL_BCAST ? drecv : const_cast<void*>(dsend);
    if (src_up) {
      if (hipMemcpyAsync(dst_up, src_up, send_bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(hip_fail(hipGetLastError(), "hipMemcpyAsync(host slice -> its stand-in)", __FILE__, __LINE__));
    }
    int rc = collective_on_host_meeting_ranks(c, coll, algo, root, dsend, drecv, count, dtype, op);
    if (rc == XMPI_OK && recv_host && (coll != COLL_REDUCE || c->rank == root)) {
      if (hipMemcpyAsync(recvbuf, drecv, recv_bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        rc = hip_fail(hipGetLastError(), "hipMemcpyAsync(stand-in -> host slice)", __FILE__, __LINE__);
    }
    return done(rc);
  }
  return collective_on_host_meeting_ranks(c, coll, algo, root, sendbuf, recvbuf, count, dtype, op);
}

}  // namespace xmpi

using namespace xmpi;

// XMPI_ERR_PEER out of a call that waited for a peer: say which peer, if the watchdog knows (ctl.cpp check_peers)
static int why_peer(xmpi_comm* c, int rc, const char* what) {
  if (rc == XMPI_ERR_PEER && c->ctl) set_last_error(std::string(what) + ": " + c->ctl->abort_reason());
  return rc;
}

extern "C" {

size_t xmpi_dtype_size(xmpi_dtype dtype) {
  switch (dtype) {
    case XMPI_U8: return 1;
    case XMPI_I32: return 4;
    case XMPI_I64: return 8;
    case XMPI_F16: return 2;
    case XMPI_F32: return 4;
    case XMPI_F64: return 8;
    case XMPI_BF16: return 2;
    case XMPI_F8E4M3: return 1;
    case XMPI_F8E5M2: return 1;
    default: return 0;
  }
}

const char* xmpi_version(void) { return "xmpi 0.1 (gfx950, HIP)"; }

const char* xmpi_degraded(const xmpi_comm* c) { return (c && !c->finalized) ? c->degraded_why.c_str() : ""; }

const char* xmpi_last_error(void) { return g_last_error.c_str(); }

const char* xmpi_strerror(int code) {
  switch (code) {
    case XMPI_OK: return "ok";
    case XMPI_ERR_ARG: return "invalid argument";
    case XMPI_ERR_HIP: return "HIP runtime error";
    case XMPI_ERR_BOOTSTRAP: return "bootstrap (shared control block) failed";
    case XMPI_ERR_TIMEOUT: return "timed out waiting for a peer";
    case XMPI_ERR_TAG_EXISTS: return "tag already in use";
    case XMPI_ERR_TRUNCATE: return "message larger than the receive buffer";
    case XMPI_ERR_NOMEM: return "out of memory";
    case XMPI_ERR_STATE: return "communicator not initialised";
    case XMPI_ERR_UNSUPPORTED: return "unsupported";
    case XMPI_ERR_NOGPU: return "no usable HIP device (there is no CPU fallback)";
    case XMPI_ERR_PEER: return "a peer rank failed";
    default: return "unknown xmpi error";
  }
}

int xmpi_rank(const xmpi_comm* c) { return (c && !c->finalized && c->size > 0) ? c->rank : -1; }
int xmpi_size(const xmpi_comm* c) { return (c && !c->finalized) ? c->size : 0; }
int xmpi_device(const xmpi_comm* c) { return (c && !c->finalized) ? c->device : -1; }

int xmpi_barrier(xmpi_comm* c) {
  XMPI_ENTER(c);
  drain_worker(c);
  dsync_service(c);
  Backoff bo;
  arm(bo, c);
  int rc = c->ctl->barrier(wait_limit(c), &bo);
  if (rc != XMPI_OK) set_last_error("barrier: a peer did not arrive");
  return rc;
}

void* xmpi_malloc(xmpi_comm* c, size_t bytes) {
  if (!c || c->finalized || use_device(c) != XMPI_OK) return nullptr;
  void* p = heap_alloc(c->device, bytes);  // a block of a registered arena (heap.cpp)
  if (!p) hip_fail(hipGetLastError(), "hipMalloc(arena)", __FILE__, __LINE__);
  return p;
}

int xmpi_free(xmpi_comm* c, void* p) {
  XMPI_ENTER(c);
  if (p && !heap_free(p)) {
    set_last_error("free: not a live buffer of xmpi_malloc");
    return XMPI_ERR_ARG;
  }
  return XMPI_OK;
}

int xmpi_register(xmpi_comm* c, void* p, size_t bytes) {
  XMPI_ENTER(c);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (!p || !is_device_pointer(p) || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    set_last_error("register: not a device allocation");
    return XMPI_ERR_ARG;
  }
  if ((char*)p + bytes > (char*)base + size) {
    set_last_error("register: the range runs past its allocation");
    return XMPI_ERR_ARG;
  }
  if (heap_owns(p)) return XMPI_OK;  // memory of xmpi_malloc is registered as it is
  return registry_add((void*)base, size, c->device);
}

int xmpi_deregister(xmpi_comm* c, void* p) {
  XMPI_ENTER(c);
  if (heap_owns(p)) {
    set_last_error("deregister: memory of xmpi_malloc stays registered until xmpi_free");
    return XMPI_ERR_ARG;
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (!p || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    registry_remove(c, p);
    return XMPI_OK;
  }
  registry_remove(c, (void*)base);
  return XMPI_OK;
}

int xmpi_memcpy(xmpi_comm* c, void* dst, const void* src, size_t bytes) {
  XMPI_ENTER(c);
  if (bytes) {  // on the communicator's stream (the null stream would cost the process another hardware queue)
    XMPI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->local_stream));
    XMPI_HIP(hipStreamSynchronize(c->local_stream));
  }
  return XMPI_OK;
}

int xmpi_memset(xmpi_comm* c, void* dst, int byte, size_t bytes) {
  XMPI_ENTER(c);
  if (bytes) {
    XMPI_HIP(hipMemsetAsync(dst, byte, bytes, c->local_stream));
    XMPI_HIP(hipStreamSynchronize(c->local_stream));
  }
  return XMPI_OK;
}

int xmpi_sync(xmpi_comm* c) {
  XMPI_ENTER(c);
  XMPI_HIP(hipDeviceSynchronize());
  return XMPI_OK;
}

// xmpi_send (waits for the receiver's confirmation) and xmpi_send_nowait (xmpi_wait collects it)
static int send_checked(xmpi_comm* c, const void* buf, size_t count, xmpi_dtype dtype, int dest, int tag, bool wait_ack) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || dest < 0 || dest >= c->size || (count && !buf) || tag == kVTag) {
    set_last_error("send: bad dtype / destination / buffer (or the one tag the library keeps to itself)");
    return XMPI_ERR_ARG;
  }
  return why_peer(c, p2p_send(c, buf, count * es, (int)dtype, dest, tag, wait_ack), "send");
}

int xmpi_send(xmpi_comm* c, const void* buf, size_t count, xmpi_dtype dtype, int dest, int tag) { return send_checked(c, buf, count, dtype, dest, tag, true); }
int xmpi_send_nowait(xmpi_comm* c, const void* buf, size_t count, xmpi_dtype dtype, int dest, int tag) { return send_checked(c, buf, count, dtype, dest, tag, false); }

int xmpi_wait(xmpi_comm* c, int dest, int tag) {
  XMPI_ENTER(c);
  if (dest < 0 || dest >= c->size) return XMPI_ERR_ARG;
  return why_peer(c, p2p_wait(c, dest, tag), "wait");
}

int xmpi_recv(xmpi_comm* c, void* buf, size_t capacity, xmpi_dtype dtype, int src, int tag, size_t* got) {
  XMPI_ENTER(c);
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || src < 0 || src >= c->size || (capacity && !buf) || tag == kVTag) {
    set_last_error("receive: bad dtype / source / buffer (or the one tag the library keeps to itself)");
    return XMPI_ERR_ARG;
  }
  size_t got_bytes = 0;
  int rc = p2p_recv(c, buf, capacity * es, (int)dtype, src, tag, &got_bytes);
  if (got) *got = got_bytes / es;
  return why_peer(c, rc, "receive");
}

int xmpi_probe(xmpi_comm* c, int src, int tag, size_t* count, xmpi_dtype* dtype) {
  XMPI_ENTER(c);
  if (src < 0 || src >= c->size) return XMPI_ERR_ARG;
  size_t bytes = 0;
  int dt = 0;
  int rc = p2p_probe(c, src, tag, &bytes, &dt);
  if (rc != XMPI_OK) return rc;
  const size_t es = xmpi_dtype_size((xmpi_dtype)dt);
  if (count) *count = es ? bytes / es : 0;
  if (dtype) *dtype = (xmpi_dtype)dt;
  return XMPI_OK;
}

int xmpi_bcast(xmpi_comm* c, void* buf, size_t count, xmpi_dtype dtype, int root, int algo) {
  XMPI_ENTER(c);
  return collective(c, COLL_BCAST, algo, root, buf, buf, count, (int)dtype, XMPI_SUM);
}

int xmpi_reduce(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op, int root,
                int algo) {
  XMPI_ENTER(c);
  // recvbuf is only significant at the root; other ranks may pass NULL
  void* rb = recvbuf ? recvbuf : const_cast<void*>(sendbuf);
  if (c->rank == root && !recvbuf) {
    set_last_error("reduce: root needs a receive buffer");
    return XMPI_ERR_ARG;
  }
  return collective(c, COLL_REDUCE, algo, root, sendbuf, rb, count, (int)dtype, (int)op);
}

int xmpi_allreduce(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op,
                   int algo) {
  XMPI_ENTER(c);
  return collective(c, COLL_ALLREDUCE, algo, 0, sendbuf, recvbuf, count, (int)dtype, (int)op);
}

int xmpi_allgather(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, int algo) {
  XMPI_ENTER(c);
  return collective(c, COLL_ALLGATHER, algo, 0, sendbuf, recvbuf, count, (int)dtype, XMPI_SUM);
}

int xmpi_reduce_scatter(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op, int algo) {
  XMPI_ENTER(c);
  return collective(c, COLL_REDUCE_SCATTER, algo, 0, sendbuf, recvbuf, count, (int)dtype, (int)op);
}

int xmpi_alltoall(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, int algo) {
  XMPI_ENTER(c);
  return collective(c, COLL_ALLTOALL, algo, 0, sendbuf, recvbuf, count, (int)dtype, XMPI_SUM);
}

// ---- stream-ordered forms --------------------------------------------------------------------------
static int on_stream(xmpi_comm* c, int coll, int root, const void* sendbuf, void* recvbuf, size_t count, int dtype, int op,
                     void* stream) {
  const size_t es = xmpi_dtype_size((xmpi_dtype)dtype);
  if (es == 0 || op < 0 || op >= XMPI_OP_COUNT || root < 0 || root >= c->size) {
    set_last_error("bad dtype / op / root");
    return XMPI_ERR_ARG;
  }
  if (refuse_bitwise_on_float(dtype, op)) return XMPI_ERR_ARG;  // a bitwise operator on a float type
  op = normal_op(dtype, op);
  if (count == 0) return XMPI_OK;
  if (!sendbuf || !recvbuf) {
    set_last_error("null buffer");
    return XMPI_ERR_ARG;
  }
  if (coll_personal(coll) && personal_overlap(c, coll, sendbuf, recvbuf, count * es)) return XMPI_ERR_ARG;
  drain_worker(c);
  std::lock_guard<std::mutex> g(c->coll_mu);
  hipStream_t s = stream ? (hipStream_t)stream : c->local_stream;
  if (c->size == 1) {  // a job of one: the result is the input
    if (coll != COLL_BCAST && sendbuf != recvbuf) XMPI_HIP(hipMemcpyAsync(recvbuf, sendbuf, count * es, hipMemcpyDefault, s));
    return XMPI_OK;  // (reduce-scatter, all-to-all: one block of `count` elements too)
  }
  if (!dsync_usable(c)) {
    // ranks sharing a (process, GPU) pair meet on the host (see dsync.cpp): order the call after the stream's
    // work, run it blocking.  Correct, but the host waits -- the layout this API is for is one process per GPU.
    XMPI_HIP(hipStreamSynchronize(s));
    bool done = false;
    int rc = zero_copy_collective(c, coll, root, sendbuf, recvbuf, count, dtype, op, false, &done);
    if (rc != XMPI_OK || done) return rc;
    set_last_error("stream-ordered collectives need buffers of xmpi_malloc / xmpi_register when ranks share a process and a GPU");
    return XMPI_ERR_UNSUPPORTED;
  }
  // device memory only: a copy to or from pageable host memory would block this call until the kernel before it
  // has ended, i.e. until every peer has arrived -- the opposite of what the stream-ordered forms are for
  if (!is_device_pointer(sendbuf) || !is_device_pointer(recvbuf)) {
    set_last_error("stream-ordered collectives take device memory (use the blocking forms for host buffers)");
    return XMPI_ERR_ARG;
  }
  return dsync_collective(c, coll, root, sendbuf, recvbuf, count, dtype, op, s, /*blocking=*/false, XMPI_ALGO_AUTO);
}

int xmpi_allreduce_on_stream(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op,
                             void* stream) {
  XMPI_ENTER(c);
  return on_stream(c, COLL_ALLREDUCE, 0, sendbuf, recvbuf, count, (int)dtype, (int)op, stream);
}

int xmpi_allgather_on_stream(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, void* stream) {
  XMPI_ENTER(c);
  return on_stream(c, COLL_ALLGATHER, 0, sendbuf, recvbuf, count, (int)dtype, XMPI_SUM, stream);
}

int xmpi_bcast_on_stream(xmpi_comm* c, void* buf, size_t count, xmpi_dtype dtype, int root, void* stream) {
  XMPI_ENTER(c);
  return on_stream(c, COLL_BCAST, root, buf, buf, count, (int)dtype, XMPI_SUM, stream);
}

int xmpi_reduce_on_stream(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op,
                          int root, void* stream) {
  XMPI_ENTER(c);
  void* rb = recvbuf ? recvbuf : const_cast<void*>(sendbuf);
  if (c->rank == root && !recvbuf) {
    set_last_error("reduce: root needs a receive buffer");
    return XMPI_ERR_ARG;
  }
  return on_stream(c, COLL_REDUCE, root, sendbuf, rb, count, (int)dtype, (int)op, stream);
}

int xmpi_reduce_scatter_on_stream(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op,
                                  void* stream) {
  XMPI_ENTER(c);
  return on_stream(c, COLL_REDUCE_SCATTER, 0, sendbuf, recvbuf, count, (int)dtype, (int)op, stream);
}

int xmpi_alltoall_on_stream(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, void* stream) {
  XMPI_ENTER(c);
  return on_stream(c, COLL_ALLTOALL, 0, sendbuf, recvbuf, count, (int)dtype, XMPI_SUM, stream);
}

void* xmpi_stream_create(xmpi_comm* c) {
  if (!c || c->finalized || use_device(c) != XMPI_OK) return nullptr;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
    return nullptr;
  }
  return (void*)s;
}

int xmpi_stream_destroy(xmpi_comm* c, void* stream) {
  XMPI_ENTER(c);
  if (stream) {
    std::lock_guard<std::mutex> g(c->coll_mu);
    if (c->dsync_last_stream == (hipStream_t)stream) {  // the next device-synchronised launch would order itself behind it
      (void)hipStreamSynchronize((hipStream_t)stream);
      c->dsync_last_stream = nullptr;
    }
    XMPI_HIP(hipStreamDestroy((hipStream_t)stream));
  }
  return XMPI_OK;
}

// ---- hipGraph capture of stream-ordered collectives ---------------------------------------------------------------
// A device-synchronised collective is one kernel launch whose arguments do not change from call to call on the same
// buffers (its epoch is counted on the device, DsyncPage::epoch_now), so a sequence of them -- with the caller's own
// kernels in between -- can be captured once and replayed: the launch-bound inner loop of an iterative solver becomes one
// hipGraphLaunch per iteration.  Every rank captures the same sequence and replays it the same number of times.
int xmpi_graph_begin(xmpi_comm* c, void* stream) {
  XMPI_ENTER(c);
  if (!stream) {
    set_last_error("graph capture needs a stream of the caller's (xmpi_stream_create)");
    return XMPI_ERR_ARG;
  }
  if (!dsync_usable(c)) {
    set_last_error("graph capture needs ranks that meet on the device (one process per GPU)");
    return XMPI_ERR_UNSUPPORTED;
  }
  // relaxed: other threads of this process (the helper that maps peers' buffers) may keep calling the runtime
  XMPI_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed));
  return XMPI_OK;
}

int xmpi_graph_end(xmpi_comm* c, void* stream, void** graph_out) {
  XMPI_ENTER(c);
  if (!stream || !graph_out) return XMPI_ERR_ARG;
  hipGraph_t g = nullptr;
  XMPI_HIP(hipStreamEndCapture((hipStream_t)stream, &g));
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return hip_fail(e, "hipGraphInstantiate", __FILE__, __LINE__);
  *graph_out = (void*)exec;
  return XMPI_OK;
}

int xmpi_graph_launch(xmpi_comm* c, void* graph, void* stream) {
  XMPI_ENTER(c);
  if (!graph) return XMPI_ERR_ARG;
  hipStream_t s = stream ? (hipStream_t)stream : c->local_stream;
  std::lock_guard<std::mutex> g(c->coll_mu);
  dsync_graph_launched(c, s, /*before=*/true);
  XMPI_HIP(hipGraphLaunch((hipGraphExec_t)graph, s));
  dsync_graph_launched(c, s, /*before=*/false);
  return XMPI_OK;
}

int xmpi_graph_destroy(xmpi_comm* c, void* graph) {
  XMPI_ENTER(c);
  if (graph) XMPI_HIP(hipGraphExecDestroy((hipGraphExec_t)graph));
  return XMPI_OK;
}

int xmpi_stream_sync(xmpi_comm* c, void* stream) {
  XMPI_ENTER(c);
  hipStream_t s = stream ? (hipStream_t)stream : c->local_stream;
  // poll, serving the peers meanwhile: a peer may be waiting for this rank to map a buffer it just registered
  hipEvent_t fin = ev_get(c, false);
  if (!fin) return XMPI_ERR_HIP;
  XMPI_HIP(hipEventRecord(fin, s));
  Backoff bo;
  arm(bo, c);
  for (;;) {
    const hipError_t e = hipEventQuery(fin);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery", __FILE__, __LINE__);
    (void)hipGetLastError();
    bo.pause();
  }
  ev_put(c, fin, false);
  std::lock_guard<std::mutex> g(c->coll_mu);
  const int prc = c->dsync_ok ? dsync_p2p_reap(c) : XMPI_OK;  // the stream-ordered sends / receives that have completed
  const int crc = dsync_check(c);
  if (crc == XMPI_OK && prc == XMPI_ERR_PEER) set_last_error("send / receive: the job was aborted while the kernel waited: " + c->ctl->abort_reason());
  return crc != XMPI_OK ? crc : prc;
}

// ---- stream-ordered Send / Receive ----------------------------------------------------------------------------------
static int p2p_on_stream_ok(xmpi_comm* c, const void* buf, size_t count, xmpi_dtype dtype, int peer) {
  const size_t es = xmpi_dtype_size(dtype);
  if (!es || peer < 0 || peer >= c->size || (count && !buf)) {
    set_last_error("send / receive: bad dtype / peer / buffer");
    return XMPI_ERR_ARG;
  }
  if (!c->dsync_ok || !c->dpage) {
    set_last_error("stream-ordered send / receive need ranks that meet on the device (one process per GPU)");
    return XMPI_ERR_UNSUPPORTED;
  }
  if (count && !is_device_pointer(buf)) {
    set_last_error("stream-ordered send / receive take device memory (use the blocking forms for host buffers)");
    return XMPI_ERR_ARG;
  }
  return XMPI_OK;
}

int xmpi_send_on_stream(xmpi_comm* c, const void* buf, size_t count, xmpi_dtype dtype, int dest, int tag, void* stream) {
  XMPI_ENTER(c);
  const int rc = p2p_on_stream_ok(c, buf, count, dtype, dest);
  if (rc != XMPI_OK) return rc;
  std::lock_guard<std::mutex> g(c->coll_mu);
  return dsync_send(c, buf, count * xmpi_dtype_size(dtype), (int)dtype, dest, tag, (hipStream_t)stream);
}

int xmpi_recv_on_stream(xmpi_comm* c, void* buf, size_t capacity, xmpi_dtype dtype, int src, int tag, void* stream) {
  XMPI_ENTER(c);
  const int rc = p2p_on_stream_ok(c, buf, capacity, dtype, src);
  if (rc != XMPI_OK) return rc;
  std::lock_guard<std::mutex> g(c->coll_mu);
  return dsync_recv(c, buf, capacity * xmpi_dtype_size(dtype), (int)dtype, src, tag, (hipStream_t)stream);
}

int xmpi_iallreduce(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op, int algo,
                    xmpi_request** req) {
  XMPI_ENTER(c);
  if (!req) return XMPI_ERR_ARG;
  // (a bitwise operator on a float type: refused here, from the arguments, not by the worker)
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  *req = submit(c, [=] { return xmpi_allreduce(c, sendbuf, recvbuf, count, dtype, op, algo); });
  return XMPI_OK;
}

int xmpi_iallgather(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, int algo,
                    xmpi_request** req) {
  XMPI_ENTER(c);
  if (!req) return XMPI_ERR_ARG;
  *req = submit(c, [=] { return xmpi_allgather(c, sendbuf, recvbuf, count, dtype, algo); });
  return XMPI_OK;
}

int xmpi_ibcast(xmpi_comm* c, void* buf, size_t count, xmpi_dtype dtype, int root, int algo, xmpi_request** req) {
  XMPI_ENTER(c);
  if (!req) return XMPI_ERR_ARG;
  *req = submit(c, [=] { return xmpi_bcast(c, buf, count, dtype, root, algo); });
  return XMPI_OK;
}

int xmpi_ireduce(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op, int root,
                 int algo, xmpi_request** req) {
  XMPI_ENTER(c);
  if (!req) return XMPI_ERR_ARG;
  // (a bitwise operator on a float type: refused here, from the arguments, not by the worker)
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  *req = submit(c, [=] { return xmpi_reduce(c, sendbuf, recvbuf, count, dtype, op, root, algo); });
  return XMPI_OK;
}

int xmpi_request_test(xmpi_request* r, int* done) {
  if (!r || !done) return XMPI_ERR_ARG;
  std::lock_guard<std::mutex> l(r->mu);
  *done = r->done ? 1 : 0;
  return XMPI_OK;
}

int xmpi_request_wait(xmpi_request* r) {
  if (!r) return XMPI_ERR_ARG;
  int rc;
  {
    std::unique_lock<std::mutex> l(r->mu);
    r->cv.wait(l, [r] { return r->done; });
    rc = r->rc;
    if (rc != XMPI_OK) set_last_error(r->err);
  }
  delete r;
  return rc;
}

int xmpi_allreduce_repeat(xmpi_comm* c, const void* sendbuf, void* recvbuf, size_t count, xmpi_dtype dtype, xmpi_op op,
                          int algo, int iters) {
  XMPI_ENTER(c);
  if (refuse_bitwise_on_float((int)dtype, (int)op)) return XMPI_ERR_ARG;
  if (op >= 0 && op < XMPI_OP_COUNT) op = (xmpi_op)normal_op((int)dtype, (int)op);
  // (XMPI_SUM_WIDE, or an 8-bit float type, on a stepped schedule: refused by collective() below, from the arguments alone)
  const bool wide_stepped = fold_only((int)dtype, (int)op) && algo_stepped(algo);
  // Ranks that meet on the device: the steps are ENQUEUED back to back on the communicator's stream and waited for
  // once -- what a stream-ordered caller does, and what the device rendezvous is for (no host round trip per
  // step).  Sampled launches carry their own events, read when the last step has been waited for.
  const bool on_device = count > 0 && sendbuf && recvbuf && xmpi_dtype_size(dtype) && op >= 0 && op < XMPI_OP_COUNT && algo >= 0 && algo < XMPI_ALGO_COUNT && !wide_stepped &&
                         dsync_takes(c, COLL_ALLREDUCE, algo) && is_device_pointer(sendbuf) && is_device_pointer(recvbuf);
  if (on_device) {
    drain_worker(c);
    std::lock_guard<std::mutex> g(c->coll_mu);
    for (int i = 0; i < iters; i++) {
      const int rc = dsync_collective(c, COLL_ALLREDUCE, 0, sendbuf, recvbuf, count, (int)dtype, (int)op, c->local_stream,
                                      /*blocking=*/i == iters - 1, algo);
      if (rc != XMPI_OK) return rc;
    }
    return XMPI_OK;
  }
  // Every rank of the job a thread of this process on this GPU (bench.py on a 1-GPU box): they share one in-order
  // stream and one launch folds everybody's chunks, so K steps are K launches enqueued back to back between two
  // rendezvous instead of K x (rendezvous, launch, wait, rendezvous).  Anything the zero-copy path cannot take
  // (unregistered buffers) falls through to the step-by-step loop -- on every rank alike, the decision is collective.
  const bool all_coloc = c->shared_stream && c->zc_group_launch && c->size > 1 && iters > 1 && all_peers_colocated(c);
  int first = 0;
  if (all_coloc && count > 0 && sendbuf && recvbuf && xmpi_dtype_size(dtype) && op >= 0 && op < XMPI_OP_COUNT &&
      (algo == XMPI_ALGO_ZCOPY || (algo == XMPI_ALGO_AUTO && c->zero_copy))) {
    drain_worker(c);
    std::lock_guard<std::mutex> g(c->coll_mu);
    bool done = false;
    const int rc = zero_copy_collective(c, COLL_ALLREDUCE, 0, sendbuf, recvbuf, count, (int)dtype, (int)op, false, &done, iters);
    if (rc != XMPI_OK || done) return rc;
    first = 0;  // went staged (collectively): run the steps one by one
  }
  for (int i = first; i < iters; i++) {
    const int rc = collective(c, COLL_ALLREDUCE, algo, 0, sendbuf, recvbuf, count, (int)dtype, (int)op);
    if (rc != XMPI_OK) return rc;
  }
  return XMPI_OK;
}

int xmpi_heap_selftest(uint64_t seed, int rounds) { return heap_selftest(seed, rounds); }

}  // extern "C"
