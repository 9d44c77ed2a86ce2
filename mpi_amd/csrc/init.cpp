// init.cpp -- xmpi_init, xmpi_finalize and the one list of what a communicator owns.
#include <unistd.h>

#include <cstring>
#include <string>

#include "comm.h"
#include "kernels.h"

namespace xmpi {
namespace {

// device words, zeroed on the stream (null: no memory)
void* zeroed_device_words(size_t bytes, hipStream_t s) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) == hipSuccess) (void)hipMemsetAsync(p, 0, bytes, s);
  else p = nullptr;
  (void)hipGetLastError();
  return p;
}

// What a communicator owns goes back in two halves, every member null-checked (safe on a half-built communicator): xmpi_finalize
// has a job barrier between them, so that nobody unmaps what a peer may still write; xmpi_init's failure exit calls them back to back.
// First: mappings, streams, events.  What came from the per-process pools goes back there (a later xmpi_init in this process finds
// it); dsync_finalize stops the helper (it reads the control block), closes the peers' flag pages, frees the pinned tables and gives
// the page back.
void release_mappings_and_streams(xmpi_comm* c) {
  zc_close_peers(c);
  dsync_finalize(c);
  for (int p = 0; p < c->size; p++) {
    if (c->peer_opened[p]) ipc_close_shared(c->peer_window[p]);
    if (c->shared_stream) continue;  // the per-device shared stream outlives communicators
    stream_release(c->device, c->send_stream[p]);
    stream_release(c->device, c->recv_stream[p]);
  }
  if (!c->shared_stream) {
    stream_release(c->device, c->local_stream);
    stream_release(c->device, c->batch_send_stream);
    stream_release(c->device, c->batch_recv_stream);
  }
  for (hipStream_t s : c->p2p_streams) stream_release(c->device, s);
  if (c->agent_stream) stream_release(c->device, c->agent_stream);
  if (c->ll_agent_stream) stream_release(c->device, c->ll_agent_stream);
  for (hipEvent_t e : c->ev_free) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_timed_free) (void)hipEventDestroy(e);
}

// ... then the control block's registration, the pinned and device words, the window and the scratch buffers
void release_memory(xmpi_comm* c) {
  if (c->ctl_registered) (void)hipHostUnregister(c->ctl->base());
  if (c->p2p_tickets) (void)hipFree(c->p2p_tickets);
  if (c->p2p_done) (void)hipHostFree(c->p2p_done);
  if (c->p2p_cmd) (void)hipHostFree(c->p2p_cmd);
  if (c->p2p_bounce) (void)hipHostFree(c->p2p_bounce);  // (p2p.cpp recv_direct_to_host: device -> host slice through pinned memory)
  c->p2p_bounce = c->p2p_bounce_dev = nullptr;
  if (c->p2p_rec) (void)hipFree(c->p2p_rec);
  if (c->window) pool_release(c->window);  // exported memory is never given back by the runtime: the next communicator reuses it
  if (c->temp) (void)hipFree(c->temp);
  if (c->host_stage) (void)hipFree(c->host_stage);
  if (c->dev_words) (void)hipFree(c->dev_words);
  (void)hipGetLastError();
}

// ---- xmpi_init, step by step in the order they run; each returns an xmpi error code ------------------------------------------

int pick_device(int rank, int size, int* device, xmpi_comm** out) {
  if (!out || size < 1 || size > kMaxRanks || rank < 0 || rank >= size) {
    set_last_error("xmpi_init: bad rank/size/out");
    return XMPI_ERR_ARG;
  }
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    set_last_error("xmpi_init: no HIP device is visible; xmpi has no CPU fallback");
    return XMPI_ERR_NOGPU;
  }
  if (*device < 0) *device = rank % ndev;
  if (*device >= ndev) {
    set_last_error("xmpi_init: device " + std::to_string(*device) + " does not exist (" + std::to_string(ndev) + " visible)");
    return XMPI_ERR_ARG;
  }
  XMPI_HIP(hipSetDevice(*device));
  return XMPI_OK;
}

// the control block: rank 0's layout is the job's.  Nothing to give back when this fails.
int join_job(int rank, int size, int device, const char* job_key, double limit, xmpi_comm** out) {
  CtlConfig cfg;
  cfg.lanes = (int32_t)param_env("XMPI_LANES");
  cfg.fifo_depth = (int32_t)param_env("XMPI_FIFO_DEPTH");
  cfg.slot_bytes = (uint64_t)param_env("XMPI_SLOT_BYTES") / 256 * 256;
  cfg.p2p_depth = (int32_t)param_env("XMPI_P2P_DEPTH");
  cfg.p2p_slot_bytes = (uint64_t)param_env("XMPI_P2P_SLOT_BYTES") / 256 * 256;
  cfg.host_lane_bytes = param_env("XMPI_HOST_LANES");  // a request: the creator of the block sizes and reserves them
  XMPI_TRACE_STEP(rank, "init: joining the control block");
  std::string key = (job_key && *job_key) ? job_key : "default";
  std::string err;
  Ctl* ctl = nullptr;
  int rc = Ctl::join(key, rank, size, cfg, limit, &ctl, &err);
  if (rc != XMPI_OK) {
    set_last_error("xmpi_init: " + err);
    return rc;
  }
  XMPI_TRACE_STEP(rank, "init: joined");
  xmpi_comm* c = new xmpi_comm;
  c->rank = rank;
  c->size = size;
  c->device = device;
  c->ctl = ctl;
  const CtlConfig& g = ctl->cfg();  // rank 0's values are the job's
  c->lanes = g.lanes;
  c->fifo_depth = g.fifo_depth;
  c->slot_bytes = g.slot_bytes;
  c->p2p_depth = g.p2p_depth;
  c->p2p_slot_bytes = g.p2p_slot_bytes;
  c->coll_region_bytes = (size_t)size * c->lanes * c->fifo_depth * c->slot_bytes;
  c->window_bytes = c->coll_region_bytes + (size_t)size * kMailEntries * c->p2p_depth * c->p2p_slot_bytes;
  memset(c->tune_algo, -1, sizeof c->tune_algo);
  memset(c->tune_split, -1, sizeof c->tune_split);
  memset(c->tune_unroll, 0, sizeof c->tune_unroll);
  params_from_env(c);  // every row of the table (params.cpp) whose default does not wait for the job's layout; those: where it is known
  c->ll_agent_us = param_env("XMPI_LL_AGENT_US", c->p2p_agent_us);
  *out = c;
  return XMPI_OK;
}

// this rank's window, its handle, its stream and its flag page; published; then every peer has published its own
int publish_window(xmpi_comm* c, double limit) {
  XMPI_TRACE_STEP(c->rank, "init: window");
  c->window = (char*)pool_acquire(c->device, c->window_bytes, 0, nullptr, nullptr);
  if (!c->window) {
    hip_fail(hipGetLastError(), "hipMalloc(window)", __FILE__, __LINE__);
    return XMPI_ERR_NOMEM;
  }
  RankInfo* me = c->ctl->info(c->rank);
  me->device = c->device;
  me->maps = 0;
  me->maps_why[0] = 0;
  me->window_addr = (uint64_t)(uintptr_t)c->window;
  me->window_bytes = c->window_bytes;
  (void)hipDeviceGetPCIBusId(me->busid, (int)sizeof me->busid, c->device);
  if (c->size > 1) {
    hipIpcMemHandle_t h;
    hipError_t e = pool_handle(c->window, &h);
    if (e != hipSuccess) {
      hip_fail(e, "hipIpcGetMemHandle", __FILE__, __LINE__);
      return XMPI_ERR_HIP;
    }
    static_assert(sizeof(h) <= sizeof(me->ipc_handle), "ipc handle size");
    memcpy(me->ipc_handle, &h, sizeof h);
  }
  XMPI_TRACE_STEP(c->rank, "init: stream");
  // this rank's stream, before anything is enqueued anywhere (the null stream would cost a second hardware queue)
  c->local_stream = stream_acquire(c->device);
  if (!c->local_stream) {
    hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
    return XMPI_ERR_HIP;
  }
  XMPI_TRACE_STEP(c->rank, "init: flag page");
  (void)dsync_prepare(c);  // this rank's flag page (device-synchronised collectives), published with the window
  XMPI_TRACE_STEP(c->rank, "init: published, waiting for the peers' windows");
  me->state.store(2, std::memory_order_release);
  int rc = c->ctl->wait_all_state(2, limit);
  if (rc != XMPI_OK) set_last_error("xmpi_init: a peer did not publish its HBM window");
  return rc;
}

int map_peer_windows(xmpi_comm* c) {
  XMPI_TRACE_STEP(c->rank, "init: mapping the peers' windows");
  RankInfo* me = c->ctl->info(c->rank);
  const int mypid = (int)getpid();
  for (int p = 0; p < c->size; p++) {
    if (p == c->rank) {
      c->peer_window[p] = c->window;
      continue;
    }
    RankInfo* pi = c->ctl->info(p);
    if (pi->pid == mypid) {  // rank hosted by a thread of this process
      c->peer_window[p] = (char*)(uintptr_t)pi->window_addr;
      if (pi->device != c->device) {
        hipError_t e = hipDeviceEnablePeerAccess(pi->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
          hip_fail(e, "hipDeviceEnablePeerAccess", __FILE__, __LINE__);
          return XMPI_ERR_HIP;
        }
        (void)hipGetLastError();
      }
    } else {
      void* ptr = nullptr;
      hipError_t e = ipc_open_shared(pi->pid, pi->window_addr, pi->ipc_handle, &ptr);
      if (e != hipSuccess) {
        // not the end of the job: this rank says so in the vote below (dsync_connect) and every rank keeps to what does not need
        // the windows -- the device-synchronised collectives on registered buffers, Send / Receive out of registered buffers
        // and through the host lanes
        (void)hipGetLastError();
        if (!c->window_map_failed)
          snprintf(me->maps_why, sizeof me->maps_why, "rank %d: hipIpcOpenMemHandle(window of rank %d): %s", c->rank, p, hipGetErrorString(e));
        c->window_map_failed = true;
        continue;
      }
      c->peer_window[p] = (char*)ptr;
      c->peer_opened[p] = true;
    }
  }
  return XMPI_OK;
}

// Ranks hosted by threads of one process on one GPU share a single in-order stream: HBM is their
// only shared resource, so concurrent streams would only make every kernel slower, while one
// stream lets each kernel run at full-chip bandwidth (and needs no cross-stream events).
// Otherwise ONE stream (publish_window's); the per-peer streams of the staged schedules are made when a staged schedule
// first runs (ensure_streams).  Every stream costs the process a hardware queue (the runtime multiplexes streams
// over GPU_MAX_HW_QUEUES of them), and a GPU runs only a few dozen queues at once: 8 processes x 4 queues on one
// GPU were time-sliced by the scheduler -- 22 ms per collective instead of 40 us (profiles/r02).
int choose_streams(xmpi_comm* c) {
  const int mypid = (int)getpid();
  bool colocated = false;
  for (int p = 0; p < c->size; p++)
    if (p != c->rank && c->ctl->info(p)->pid == mypid && c->ctl->info(p)->device == c->device) {
      colocated = true;
      c->peer_coloc[p] = true;
    }
  const long shared_env = param_env("XMPI_SHARED_STREAM");
  c->shared_stream = shared_env < 0 ? colocated : shared_env != 0;
  if (!c->shared_stream) return XMPI_OK;
  hipStream_t s = shared_stream_for(c->device);
  if (!s) {
    c->shared_stream = false;  // (the stream of its own goes back to the pool)
    hip_fail(hipGetLastError(), "hipStreamCreate(shared)", __FILE__, __LINE__);
    return XMPI_ERR_HIP;
  }
  for (int p = 0; p < c->size; p++) c->send_stream[p] = c->recv_stream[p] = (p == c->rank) ? nullptr : s;
  (void)hipStreamSynchronize(c->local_stream);
  stream_release(c->device, c->local_stream);
  c->local_stream = c->batch_send_stream = c->batch_recv_stream = s;
  return XMPI_OK;
}

// the control block as the GPU sees it: kernels read the job's abort flag there and write the ack of a
// point-to-point message straight into its mail entry (p2p.cpp)
// (with the host lanes behind it, so that a lane's piece is copied to a device destination by DMA; the control
// structures alone if the runtime will not pin that much); and the words GPU and host pass each other.  None of it is fatal.
void map_control_words(xmpi_comm* c) {
  Ctl* ctl = c->ctl;
  if (ctl->host_lane_bytes() > 0 && hipHostRegister(ctl->base(), ctl->bytes(), hipHostRegisterMapped) == hipSuccess) c->lanes_dev_ok = true;
  if (c->lanes_dev_ok ||
      ((void)hipGetLastError(), hipHostRegister(ctl->base(), Ctl::layout_bytes(c->size), hipHostRegisterMapped) == hipSuccess)) {
    c->ctl_registered = true;
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, ctl->base(), 0) == hipSuccess) c->ctl_dev = (char*)dev;
  }
  if (!c->ctl_dev) c->lanes_dev_ok = false;
  (void)hipGetLastError();
  // (two more for the copy kernels that carry a host slice into / out of a collective's stand-in, dsync.cpp)
  c->p2p_tickets = (uint32_t*)zeroed_device_words((xmpi_comm::kP2PDoneSlots + 2) * sizeof(uint32_t), c->local_stream);
  // completion words the GPU writes and a host thread polls (stream-ordered Send / Receive: slots 0..63; the pull kernels
  // of the blocking Receive: 64..127)
  pinned_words(sizeof(uint64_t) * 4 * 2 * xmpi_comm::kP2PDoneSlots, &c->p2p_done, &c->p2p_done_dev);
  pinned_words(128, &c->p2p_cmd, &c->p2p_cmd_dev);  // (two records: the receive agent's, the LL agent's)
  if (c->p2p_cmd_dev) {
    c->ll_cmd = c->p2p_cmd + 8;
    c->ll_cmd_dev = c->p2p_cmd_dev + 8;
  }
  c->p2p_rec = (uint64_t*)zeroed_device_words(64, c->local_stream);
}

// flag pages, the helper thread, what depends on the layout they found, and the bootstrap's last barrier
int connect_and_meet(xmpi_comm* c, double limit) {
  Ctl* ctl = c->ctl;
  XMPI_TRACE_STEP(c->rank, "init: connecting flag pages");
  int rc = dsync_connect(c, limit);
  if (rc != XMPI_OK) return rc;
  // the helper thread: maps what peers register, and watches over their processes -- unless one of them cannot be seen from here
  // even now, when it certainly lives (ranks in different pid namespaces sharing /dev/shm: no way to ask, so nobody asks)
  for (int p = 0; p < c->size && c->watchdog_ms > 0; p++)
    if (p != c->rank && ctl->peer_gone(p)) c->watchdog_ms = 0;
  ctl->set_watch(c->watchdog_ms > 0);
  dsync_start_helper(c);
  XMPI_TRACE_STEP(c->rank, "init: final barrier");
  c->dsync_unroll = param_env("XMPI_DSYNC_UNROLL", c->dsync_sharers > 1 ? 1 : 2);
  // ranks sharing a GPU: fewer, longer blocks (8 processes on one MI355X: 4 MiB 170 -> 90 us, 16 MiB 231 -> 169 us);
  // a rank with a GPU to itself keeps one tile per block -- over links more waves in flight is what hides latency
  c->dsync_tiles = param_env("XMPI_DSYNC_TILES", c->dsync_sharers > 1 ? 8 : 1);
  if (hipMalloc((void**)&c->dev_words, 4 * sizeof(uint64_t)) != hipSuccess) {
    hip_fail(hipGetLastError(), "hipStreamCreate/hipMalloc", __FILE__, __LINE__);
    return XMPI_ERR_HIP;
  }
  {  // before the barrier: no rank of this process can allocate before every one of them has said so
    bool shared = false;
    for (int p = 0; p < c->size; p++) shared = shared || (p != c->rank && ctl->info(p)->pid == (int32_t)getpid());
    heap_colour_seed(c->rank, shared);
  }
  rc = ctl->barrier(limit);
  if (rc != XMPI_OK) set_last_error("xmpi_init: barrier failed");
  return rc;
}

// The ranks sit on different GPUs (or XMPI_SELFCHECK=1): what untuned AUTO can reach is tried on patterned inputs before the
// first caller's data goes through it (tune.cpp init_selfcheck).  A job that tunes right here checks every candidate anyway.
// XMPI_AUTOTUNE_BYTES=N: the library times its schedules for messages up to N bytes right here (xmpi_tune), so that a
// program that knows nothing about tuning gets the schedule a benchmark would pick on this node; every rank sees the
// same environment, so it is collective.  Default: off (a few hundred milliseconds and 2 x N bytes of HBM per rank).
int check_or_tune(xmpi_comm* c) {
  const long tune_bytes = env_long("XMPI_AUTOTUNE_BYTES", 0);
  if (c->selfcheck < 0) {
    const RankInfo* me = c->ctl->info(c->rank);
    bool spread = false;
    for (int p = 0; p < c->size; p++) spread = spread || strncmp(c->ctl->info(p)->busid, me->busid, sizeof me->busid) != 0;
    c->selfcheck = spread ? 1 : 0;
  }
  int rc = XMPI_OK;
  if (c->selfcheck && dsync_usable(c) && !(tune_bytes > 0)) {
    XMPI_TRACE_STEP(c->rank, "init: self-check");
    rc = init_selfcheck(c);
  }
  if (rc == XMPI_OK && tune_bytes > 0 && c->size > 1) {
    XMPI_TRACE_STEP(c->rank, "init: tuning");
    rc = xmpi_tune(c, (size_t)tune_bytes);
  }
  return rc;
}

}  // namespace
}  // namespace xmpi

using namespace xmpi;

extern "C" {

int xmpi_init(int rank, int size, int device, const char* job_key, xmpi_comm** out) {
  int rc = pick_device(rank, size, &device, out);
  if (rc != XMPI_OK) return rc;
  // Two different clocks.  XMPI_INIT_TIMEOUT_S (default 60; 0 or less: an hour) bounds the bootstrap only -- the reference's
  // -mpi-inittimeout (network.go:223-234,307-312).  XMPI_TIMEOUT_S is the no-progress limit of Send / Receive and
  // the collectives afterwards: default 0 = wait for ever, as the reference's blocking calls do (a receiver may
  // compute for minutes before it posts its Receive); tests set it so a bug shows up as an error, not a hang.
  const double timeout = (double)env_long("XMPI_INIT_TIMEOUT_S", 60), limit = timeout > 0 ? timeout : 3600.0;
  xmpi_comm* c = nullptr;
  rc = join_job(rank, size, device, job_key, limit, &c);
  if (rc != XMPI_OK) return rc;
  rc = publish_window(c, limit);
  if (rc == XMPI_OK) rc = map_peer_windows(c);
  if (rc == XMPI_OK) rc = choose_streams(c);
  if (rc == XMPI_OK) {
    map_control_words(c);
    rc = connect_and_meet(c, limit);
  }
  if (rc != XMPI_OK) {  // the one failure exit of the bootstrap: no barrier (the peers see the abort), no heap_comm_destroyed (nothing created)
    c->ctl->set_abort(rc);
    release_mappings_and_streams(c);
    release_memory(c);
    delete c->ctl;
    delete c;
    return rc;
  }
  heap_comm_created();
  rc = check_or_tune(c);
  if (rc != XMPI_OK) {
    (void)xmpi_finalize(c);
    return rc;
  }
  XMPI_TRACE_STEP(rank, "init: done");
  *out = c;
  return XMPI_OK;
}

int xmpi_finalize(xmpi_comm* c) {
  if (!c) return XMPI_ERR_STATE;
  if (c->finalized) return XMPI_OK;
  stop_worker(c);  // outstanding non-blocking collectives complete first
  p2p_agent_stop(c);  // the receive agent (if it still lingers) is told to go
  ll_agent_stop(c);   // ... and the LL agent
  XMPI_TRACE_STEP(c->rank, "finalize: device sync");
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  XMPI_TRACE_STEP(c->rank, "finalize: barrier");
  // nobody may still be writing into a window that is about to be unmapped
  if (!c->ctl->aborted()) {
    Backoff bo;
    arm(bo, c);
    (void)c->ctl->barrier(wait_limit(c), &bo);
  }
  XMPI_TRACE_STEP(c->rank, "finalize: closing");
  release_mappings_and_streams(c);
  if (!c->ctl->aborted()) (void)c->ctl->barrier(wait_limit(c));
  release_memory(c);
  heap_comm_destroyed(c);  // last communicator of the process: empty arenas go back to the device
  XMPI_TRACE_STEP(c->rank, "finalize: done");
  c->ctl->info(c->rank)->state.store(3, std::memory_order_release);
  delete c->ctl;
  c->ctl = nullptr;
  c->finalized = true;
  delete c;
  return XMPI_OK;
}

}  // extern "C"
