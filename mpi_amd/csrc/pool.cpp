// pool.cpp -- what outlives a communicator: the mappings of peers' blocks, the exported blocks and the streams, per process.
#include <signal.h>

#include <cerrno>
#include <cstring>
#include <mutex>
#include <vector>

#include "comm.h"

namespace xmpi {

// ---- windows and their mappings outlive communicators (shared with dsync.cpp) -----------------------------------------------
// Measured on MI355X / ROCm 7.2: memory that was exported with hipIpcGetMemHandle and mapped by another process
// is NOT given back by hipFree + hipIpcCloseMemHandle while both processes live -- 8 ranks that create and
// finalise a communicator in a loop lost 10 GiB of HBM per lifetime (8 windows of 1.25 GiB) and ran out after 27.
// So nothing of that kind is freed or unmapped per communicator any more: a finalised communicator's window (and
// flag page) goes into a per-process pool and the next communicator of that size takes it from there; a peer's
// mapping of it stays open and is found again by {owner pid, address, handle}.  This also removes the one moment
// where a stray write could meet an unmapped page ("the round-1 fault").
struct IpcMapping {
  int owner_pid;
  uint64_t owner_addr;
  uint8_t handle[64];
  void* ptr;
  int refs;
};
static std::mutex g_ipc_mu;
static std::vector<IpcMapping> g_ipc_map;

hipError_t ipc_open_shared(int owner_pid, uint64_t owner_addr, const void* handle_bytes, void** out) {
  std::lock_guard<std::mutex> g(g_ipc_mu);
  for (size_t i = 0; i < g_ipc_map.size(); i++) {
    IpcMapping& m = g_ipc_map[i];
    if (m.owner_pid != owner_pid || m.owner_addr != owner_addr) continue;
    if (memcmp(m.handle, handle_bytes, sizeof(hipIpcMemHandle_t)) == 0) {
      m.refs++;
      *out = m.ptr;
      return hipSuccess;
    }
    if (m.refs == 0) {  // the owner has put another allocation at that address: the old mapping is dead
      (void)hipIpcCloseMemHandle(m.ptr);
      (void)hipGetLastError();
      g_ipc_map.erase(g_ipc_map.begin() + (long)i);
    }
    break;
  }
  hipIpcMemHandle_t h;
  memcpy(&h, handle_bytes, sizeof h);
  void* ptr = nullptr;
  hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) return e;
  IpcMapping m;
  m.owner_pid = owner_pid;
  m.owner_addr = owner_addr;
  memset(m.handle, 0, sizeof m.handle);
  memcpy(m.handle, handle_bytes, sizeof h);
  m.ptr = ptr;
  m.refs = 1;
  g_ipc_map.push_back(m);
  *out = ptr;
  return hipSuccess;
}

// the mapping stays open (see above); mappings of processes that no longer exist are closed
void ipc_close_shared(void* ptr) {
  std::lock_guard<std::mutex> g(g_ipc_mu);
  for (IpcMapping& m : g_ipc_map)
    if (m.ptr == ptr && m.refs > 0) {
      m.refs--;
      break;
    }
  for (size_t i = 0; i < g_ipc_map.size();) {
    IpcMapping& m = g_ipc_map[i];
    if (m.refs == 0 && kill(m.owner_pid, 0) != 0 && errno == ESRCH) {
      (void)hipIpcCloseMemHandle(m.ptr);
      (void)hipGetLastError();
      g_ipc_map.erase(g_ipc_map.begin() + (long)i);
    } else {
      i++;
    }
  }
}

struct PooledBlock {
  int device;
  size_t bytes;
  int kind;  // 0 = window (hipMalloc), 1 = flag page (uncached)
  void* ptr;
  bool in_use;
  bool have_handle;
  hipIpcMemHandle_t handle;
  uint64_t mark;  // what the last user left behind for the next one (flag pages: the last epoch written into it)
};
static std::mutex g_pool_mu;
static std::vector<PooledBlock> g_pool;

// HBM that peers map: taken from the pool of blocks earlier communicators of this process left behind, or
// allocated (kind 1: uncached / fine-grained, for flag words polled by kernels)
void* pool_acquire(int device, size_t bytes, int kind, bool* fresh, uint64_t* mark) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  if (fresh) *fresh = false;
  if (mark) *mark = 0;
  for (PooledBlock& b : g_pool)
    if (!b.in_use && b.device == device && b.bytes == bytes && b.kind == kind) {
      b.in_use = true;
      if (mark) *mark = b.mark;
      return b.ptr;
    }
  if (fresh) *fresh = true;
  void* p = nullptr;
  hipError_t e;
  if (kind == 1) {
    e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained);
    }
  } else {
    e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {  // memory is tight: give idle blocks of other sizes back first
      (void)hipGetLastError();
      for (size_t i = 0; i < g_pool.size();)
        if (!g_pool[i].in_use && g_pool[i].device == device) {
          (void)hipFree(g_pool[i].ptr);
          g_pool.erase(g_pool.begin() + (long)i);
        } else {
          i++;
        }
      e = hipMalloc(&p, bytes);
    }
  }
  if (e != hipSuccess) return nullptr;
  PooledBlock nb;
  memset(&nb, 0, sizeof nb);
  nb.device = device;
  nb.bytes = bytes;
  nb.kind = kind;
  nb.ptr = p;
  nb.in_use = true;
  g_pool.push_back(nb);
  return p;
}

// The hipIpc handle of a pooled block: exported ONCE, so that a peer recognises the block when a later
// communicator offers it again and keeps using the mapping it has (closing and re-opening mappings while other
// processes do the same is what fails with "invalid device pointer" on this stack).
hipError_t pool_handle(void* ptr, void* handle_out) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  for (PooledBlock& b : g_pool)
    if (b.ptr == ptr) {
      if (!b.have_handle) {
        hipError_t e = hipIpcGetMemHandle(&b.handle, ptr);
        if (e != hipSuccess) return e;
        b.have_handle = true;
      }
      memcpy(handle_out, &b.handle, sizeof b.handle);
      return hipSuccess;
    }
  return hipErrorInvalidValue;
}

// Streams outlive communicators too.  Creating a stream's hardware queue while the GPU's queues are
// oversubscribed (several processes on one GPU, a test runner holding a context of its own) made the FIRST operation
// on a new stream take 17-32 SECONDS (lifecycle trace, profiles/README.md r02): a finalised communicator's streams go
// back to a per-process pool instead of being destroyed.
static std::mutex g_stream_mu;
static std::vector<std::pair<int, hipStream_t>> g_stream_pool;

hipStream_t stream_acquire(int device) {
  {
    std::lock_guard<std::mutex> g(g_stream_mu);
    for (size_t i = 0; i < g_stream_pool.size(); i++)
      if (g_stream_pool[i].first == device) {
        hipStream_t s = g_stream_pool[i].second;
        g_stream_pool.erase(g_stream_pool.begin() + (long)i);
        return s;
      }
  }
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return s;
}

void stream_release(int device, hipStream_t s) {
  if (!s) return;
  std::lock_guard<std::mutex> g(g_stream_mu);
  g_stream_pool.push_back({device, s});
}

void pool_release(void* ptr, uint64_t mark) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  for (PooledBlock& b : g_pool)
    if (b.ptr == ptr) {
      b.in_use = false;
      b.mark = mark;
    }
}

// the per-peer / batch streams of the staged schedules (engine.cpp), created on first use
int ensure_streams(xmpi_comm* c) {
  if (c->shared_stream || c->staged_streams) return XMPI_OK;
  bool ok = (c->batch_send_stream = stream_acquire(c->device)) && (c->batch_recv_stream = stream_acquire(c->device));
  for (int p = 0; p < c->size && ok; p++) {
    if (p == c->rank) continue;
    ok = (c->send_stream[p] = stream_acquire(c->device)) && (c->recv_stream[p] = stream_acquire(c->device));
  }
  if (!ok) return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
  c->staged_streams = true;
  return XMPI_OK;
}

hipStream_t shared_stream_for(int device) {
  static std::mutex mu;
  static std::vector<std::pair<int, hipStream_t>> streams;
  std::lock_guard<std::mutex> g(mu);
  for (auto& kv : streams)
    if (kv.first == device) return kv.second;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  streams.push_back({device, s});
  return s;
}
}  // namespace xmpi
