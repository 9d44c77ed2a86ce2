// dsync_conn.cpp -- the connection lifecycle of the device-synchronised collectives (dsync.cpp and its siblings, dsync.h): the flag page of this rank
// (dsync_prepare), the mapping of every peer's page and the tables its kernels read (dsync_connect), the helper thread that keeps
// serving the peers while the application computes (dsync_start_helper / dsync_stop_helper), the way back (dsync_finalize), and
// dsync_service -- mapping what the peers have published since this rank last looked; called from every wait loop.
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "comm.h"
#include "kernels.h"
#include "sched_steps.h"

namespace xmpi {

static_assert(sizeof(DsyncPage) <= kStepOff, "flag page");
constexpr size_t kPageBytes = kDsyncPageBytes;  // the page, the step flags of the stepped kernels, the Send / Receive boxes

// Called by xmpi_init before this rank's RankInfo is published (state 2).
int dsync_prepare(xmpi_comm* c) {
  RankInfo* me = c->ctl->info(c->rank);
  me->flag_addr = 0;
  if (c->size < 2 || !c->dsync || c->size > kDsyncRanks) return XMPI_OK;  // (more ranks than the device side is sized for: they meet on the host)
  // a rank without a flag page does not fail the job: every rank sees flag_addr == 0 and keeps to the host-synchronised path;
  // it says why (xmpi_degraded)
  auto none = [&](const char* what, hipError_t e) {
    (void)hipGetLastError();
    if (!me->maps_why[0]) snprintf(me->maps_why, sizeof me->maps_why, "rank %d: %s: %s", c->rank, what, hipGetErrorString(e));
    return XMPI_OK;
  };
  // uncached HBM: the page is polled by this GPU and written by the others; it must never sit in an L2.
  // From the per-process pool (exported memory outlives communicators -- pool.cpp), and NOT cleared when it is
  // re-used: clearing is GPU work on a page seven other processes have mapped, and in a crowded GPU (eight ranks
  // plus a test runner with a context of its own) that one 64 KiB fill took 10-50 s.  Instead the epochs of the new
  // communicator start above everything an earlier one may have left in any rank's page (flag_epoch, dsync_connect).
  // (All but the 12.5 KiB of the Send / Receive areas, whose records are ordered by numbers that start again with every
  // communicator: one wave clears them in dsync_connect, in front of the flag self-test's kernel.)
  bool fresh = false;
  uint64_t last_epoch = 0;
  void* page = pool_acquire(c->device, kPageBytes, 1, &fresh, &last_epoch);
  if (!page) return none("hipExtMallocWithFlags(uncached flag page)", hipGetLastError());
  if (fresh) {
    hipError_t e = hipMemsetAsync(page, 0, kPageBytes, c->local_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->local_stream);
    if (e != hipSuccess) {
      pool_release(page, last_epoch);
      return none("hipMemset(flag page)", e);
    }
  }
  me->flag_epoch = last_epoch;
  hipIpcMemHandle_t h;
  const hipError_t he = pool_handle(page, &h);
  if (he != hipSuccess) {
    pool_release(page, last_epoch);
    return none("hipIpcGetMemHandle(uncached flag page)", he);
  }
  c->dpage = (DsyncPage*)page;
  static_assert(sizeof h <= sizeof me->flag_handle, "ipc handle size");
  memcpy(me->flag_handle, &h, sizeof h);
  me->flag_addr = (uint64_t)(uintptr_t)page;
  return XMPI_OK;
}

// Called by xmpi_init once every rank's RankInfo is visible.  Maps the peers' flag pages, then the job VOTES: every rank
// publishes what it could map (the peers' windows: xmpi_init; their flag pages: here), all meet at a barrier, and every rank
// reads the same answers -- the best level everybody reached:
//   every flag page mapped by everybody    the ranks meet on the device (this file)
//   otherwise                              they meet on the host (zcopy.cpp) and the staged step tables serve the rest
//   some window not mapped                 no staged step tables and no mail slots: every collective takes the device-synchronised
//                                          path, Send / Receive work out of registered buffers and through the host lanes
//   neither                                xmpi_init fails -- on EVERY rank, at once, with the reason (the reference's Init returns an
//                                          error only when the mesh cannot be built, network.go:53-65)
// xmpi_get_param("degraded") / xmpi_degraded() say which and why.
int dsync_connect(xmpi_comm* c, double timeout_s) {
  c->dsync_ok = false;
  if (c->size < 2) return XMPI_OK;
  const int N = c->size, mypid = (int)getpid();
  RankInfo* me = c->ctl->info(c->rank);
  bool usable = N <= kDsyncRanks;
  int sharers = 0, sharers_job = 1;
  for (int p = 0; p < N; p++) {
    const RankInfo* a = c->ctl->info(p);
    if (a->flag_addr == 0) usable = false;
    if (strncmp(a->busid, c->ctl->info(c->rank)->busid, sizeof a->busid) == 0) sharers++;
    int on_its_gpu = 0;  // the most crowded GPU of the job: what every rank must read alike (the stepped kernels' shape)
    for (int q = 0; q < N; q++)
      if (strncmp(a->busid, c->ctl->info(q)->busid, sizeof a->busid) == 0) on_its_gpu++;
    sharers_job = std::max(sharers_job, on_its_gpu);
    for (int q = p + 1; q < N; q++) {
      const RankInfo* b = c->ctl->info(q);
      if (a->pid == b->pid && a->device == b->device) usable = false;  // two ranks on one stream: see the header
    }
  }
  // (pinned words the kernels write: word 0 first failure of a kernel, bytes 8..15 epoch of the last kernel that ended, 16..23 the
  // blocking caller's completion word, words 6..11 XCD masks and probes, word 12 the flag self-test's answer)
  if (usable && hipHostMalloc((void**)&c->dsync_status, 64, hipHostMallocMapped) == hipSuccess) {
    memset(c->dsync_status, 0, 64);
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, c->dsync_status, 0) == hipSuccess) c->dsync_status_dev = (uint32_t*)dev;
  }
  (void)hipGetLastError();
  // the job's abort flag, readable by the GPU: a kernel that waits for a dead peer gives up
  if (c->ctl_dev) c->dsync_abort_dev = (const int32_t*)(c->ctl_dev + ((char*)&c->ctl->header()->abort_code - (char*)c->ctl->base()));
  bool mapped = usable;
  for (int p = 0; p < N && mapped; p++) {
    RankInfo* pi = c->ctl->info(p);
    if (p == c->rank) {
      c->peer_page[p] = c->dpage;
    } else if (pi->pid == mypid) {  // a thread of this process on another GPU (peer access is enabled by xmpi_init)
      c->peer_page[p] = (DsyncPage*)(uintptr_t)pi->flag_addr;
    } else {
      void* ptr = nullptr;
      hipError_t e = ipc_open_shared(pi->pid, pi->flag_addr, pi->flag_handle, &ptr);
      if (e != hipSuccess) {  // (an uncached allocation of ANOTHER device: nothing promises that the runtime opens it)
        (void)hipGetLastError();
        if (!me->maps_why[0])
          snprintf(me->maps_why, sizeof me->maps_why, "rank %d: hipIpcOpenMemHandle(flag page of rank %d): %s", c->rank, p, hipGetErrorString(e));
        mapped = false;
        break;
      }
      c->peer_page[p] = (DsyncPage*)ptr;
      c->peer_page_opened[p] = true;
    }
  }
  // A mapping that OPENS is not yet one that WORKS: an uncached allocation of another device, opened through hipIpc, has to carry
  // a peer's 8-byte store to the lane that polls it here.  Try it now, with a clock (a few seconds, inside xmpi_init), rather than
  // find out in the first collective, which by default waits for ever: every rank stores a token into every peer's page and waits
  // for theirs.  A rank whose words do not arrive votes "flags: no" below, and the job meets on the host.
  // The ranks get here after unsynchronised work (seven hipIpcOpenMemHandle calls, the registration of the control block,
  // hipMallocs): the self-test's clock is to measure whether the flags carry a store, not how far apart the ranks arrive -- so
  // they meet first.  Every rank, whatever it could map: a barrier only some ranks reach is a hang.
  {
    const int brc = c->ctl->barrier(timeout_s);
    if (brc != XMPI_OK) {
      set_last_error("xmpi_init: a peer did not reach the flag self-test");
      return brc;
    }
  }
  // The Send / Receive areas of this rank's page start out cleared (pool.cpp hands pages on as they were left): nothing in them is
  // told from an earlier communicator's records by a number that would have to grow.  Behind the barrier above no peer of an
  // earlier communicator writes here any more, and none of this one does before the vote below.  (XMPI_TEST_P2P_SEQ0 = S, tests:
  // the areas as S messages per ordered pair, all consumed and answered, leave them.)
  const uint64_t seq0 = (uint64_t)param_env("XMPI_TEST_P2P_SEQ0");
  if (mapped) {
    hipError_t e = launch_p2p_reset(c->dpage, seq0, c->local_stream);
    if (e == hipSuccess && !c->dsync_status_dev) e = hipStreamSynchronize(c->local_stream);  // (else: with the self-test behind it)
    if (e != hipSuccess) {
      (void)hipGetLastError();
      if (!me->maps_why[0]) snprintf(me->maps_why, sizeof me->maps_why, "rank %d: clearing the Send / Receive boxes: %s", c->rank, hipGetErrorString(e));
      mapped = false;
    }
  }
  if (mapped && c->dsync_status_dev) {
    uint64_t token = 0;
    for (int p = 0; p < N; p++) token = std::max(token, c->ctl->info(p)->flag_epoch);
    token += 1;  // (above every token an earlier communicator left in these never-cleared pages: dsync_finalize moves the mark on)
    c->dsync_selftest_token = token;  // ... this one included, whatever the vote below says (dsync_finalize)
    const double limit_s = std::min(5.0, std::max(1.0, timeout_s / 4));
    __atomic_store_n(c->dsync_status + 12, 0u, __ATOMIC_RELAXED);
    hipError_t e = launch_flag_selftest(c->peer_page, c->rank, N, token, (uint64_t)(limit_s * 1e8), c->dsync_abort_dev, c->dsync_status_dev + 12,
                                        c->local_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->local_stream);
    const uint32_t seen = __atomic_load_n(c->dsync_status + 12, __ATOMIC_ACQUIRE), all = N >= 32 ? ~0u : (1u << N) - 1u;
    if (e != hipSuccess || (seen & all) != all) {
      (void)hipGetLastError();
      if (!me->maps_why[0]) {
        if (e != hipSuccess) snprintf(me->maps_why, sizeof me->maps_why, "rank %d: flag self-test: %s", c->rank, hipGetErrorString(e));
        else snprintf(me->maps_why, sizeof me->maps_why, "rank %d: flag words of ranks %#x never arrived here (%.0f s)", c->rank, all & ~seen, limit_s);
      }
      mapped = false;
    }
  }
  // Untuned AUTO sends messages up to ll_bytes per rank as LL lines (ll.hip).  Measured with 2 processes (each kernel has the
  // GPU it runs on to itself, as on a node with one rank per GPU): 4.9 / 6.1 / 6.4 us enqueued at 1 / 4 / 16 KiB against
  // 8.9 / 8.8 / 9.4 for the fold; eight processes time-slicing ONE GPU: 45 / 56 / 65 against 47 / 47 / 42 (their polling lanes
  // compete with each other's stores for the one memory system) -- so ranks that share a GPU would keep LL to 1 KiB, were it not for the agent:
  // With the LL agent (ll.hip ll_agent_kernel) a BLOCKING call of up to 4 KiB needs no launch at all: eight processes on one GPU,
  // blocking allreduce 7.9 / 9.2 us at 1 / 4 KiB against 38 / 45 launched (no kernel, so nothing for eight processes' queues to be
  // time-sliced over) -- worth the 12 % an ENQUEUED 4 KiB LL collective loses to the fold there.  (The choice must not depend on
  // how a rank calls -- a blocking rank and an enqueueing one have to run the same protocol -- so it is one limit for both.)
  // What this rank sees -- the ranks on ITS GPU, ITS environment -- may differ from what a peer sees (5 ranks on 2 GPUs; a variable
  // set for one rank): LL or fold is a protocol choice, a rank that folds while its peer sends lines waits for ever.  So every
  // rank publishes its choice with its vote and the job takes the smallest.
  c->dsync_sharers = std::max(1, sharers);
  c->dsync_sharers_job = sharers_job;
  long mine = c->ll_bytes;
  if (mine < 0) mine = c->dsync_sharers > 2 ? ((c->agent_ll && c->ll_agent_us > 0) ? 4096 : 1024) : 8192;
  me->ll_choice = std::min<long>(mine, (long)kLLMaxPayload);
  me->maps = (c->window_map_failed ? 0 : kMapsWindows) | (mapped ? kMapsFlags : 0);
  int rc = c->ctl->barrier(timeout_s);  // ---- the vote: everything above is published, everything below is read by all alike
  if (rc != XMPI_OK) {
    set_last_error("xmpi_init: a peer did not reach the vote on what the job can map");
    return rc;
  }
  bool all_windows = true, all_flags = usable;
  std::string why_windows, why_flags;
  bool why_flags_witness = false;
  long ll = (long)kLLMaxPayload;
  for (int p = 0; p < N; p++) {
    const RankInfo* a = c->ctl->info(p);
    ll = std::min<long>(ll, (long)a->ll_choice);
    const std::string why(a->maps_why, strnlen(a->maps_why, sizeof a->maps_why));
    if (!(a->maps & kMapsWindows)) {
      all_windows = false;
      if (why_windows.empty()) why_windows = why.empty() ? "rank " + std::to_string(p) + " could not map a peer's window" : why;
    }
    if (usable && !(a->maps & kMapsFlags)) {
      all_flags = false;
      // (a rank that could not OPEN a page is the cause; the ranks whose self-test then waited for its words in vain are its witnesses)
      const bool witness = why.find("never arrived") != std::string::npos;
      if (why_flags.empty() || (why_flags_witness && !witness && !why.empty())) {
        why_flags = why.empty() ? "rank " + std::to_string(p) + " could not map a peer's flag page" : why;
        why_flags_witness = witness;
      }
    }
    if (!usable && c->dsync && a->flag_addr == 0 && why_flags.empty() && !why.empty()) why_flags = why;  // (it has no page to offer)
  }
  c->ll_bytes = std::max<long>(0, ll);
  c->windows_ok = all_windows;
  if (!all_flags)  // what this rank did map is of no use: nobody will write there
    for (int p = 0; p < N; p++) {
      if (c->peer_page_opened[p]) ipc_close_shared(c->peer_page[p]);
      c->peer_page_opened[p] = false;
      c->peer_page[p] = nullptr;
    }
  if (!all_windows && !all_flags) {
    set_last_error("xmpi_init: the job has no transport left: " + why_windows + (why_flags.empty() ? "" : "; " + why_flags) +
                   (usable ? "" : "; and the ranks cannot meet on the device (no flag pages, or ranks sharing a stream)"));
    return XMPI_ERR_HIP;
  }
  if (!all_windows)
    c->degraded_why = "no windows (no staged step tables, no mail slots; collectives: device-synchronised only): " + why_windows;
  if (!all_flags && !why_flags.empty())
    c->degraded_why += std::string(c->degraded_why.empty() ? "" : "; ") + "the ranks meet on the host (no device-synchronised collectives): " + why_flags;
  if (!c->degraded_why.empty() && c->rank == 0) fprintf(stderr, "xmpi: degraded: %s\n", c->degraded_why.c_str());
  if (!all_flags) return XMPI_OK;
  // the translation table {peer, slot} -> {registration number, where this process mapped it}: pinned host memory
  // the kernels read; the host is its only writer and needs no hardware queue to update it
  if (hipHostMalloc((void**)&c->dsync_table, sizeof(DsyncEntry) * kMaxRanks * kDsyncArenas, hipHostMallocMapped) != hipSuccess)
    return hip_fail(hipGetLastError(), "hipHostMalloc(translation table)", __FILE__, __LINE__);
  memset(c->dsync_table, 0, sizeof(DsyncEntry) * kMaxRanks * kDsyncArenas);
  {
    void* dev = nullptr;
    XMPI_HIP(hipHostGetDevicePointer(&dev, c->dsync_table, 0));
    c->dsync_table_dev = (const DsyncEntry*)dev;
  }
  // split form (sched.hip): what the meet kernel resolves for the data kernel, in ordinary device memory
  if (hipMalloc((void**)&c->dsync_res, sizeof(DsyncResolved)) != hipSuccess)
    return hip_fail(hipGetLastError(), "hipMalloc(resolved table)", __FILE__, __LINE__);
  if (hipEventCreateWithFlags(&c->dsync_order_ev, hipEventDisableTiming) != hipSuccess)
    return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__);
  // The split form acquires / releases once per XCD from kXcdBlocks one-wave blocks and counts on the dispatcher dealing them
  // round the XCDs.  Nothing promises that, so look: how many XCDs the GPU has (a grid that fills it) and which ones a grid of
  // kXcdBlocks reaches (status words 8, 9: pinned, zeroed above).  If the small grid misses one, the data kernel runs in its
  // system-scope form from the start (body_sys) -- and the done kernel checks every launch anyway (xcd_check).
  if (c->dsync_status_dev) {
    bool ok = launch_xcc_probe(c->dsync_status_dev + 8, 1024, c->local_stream) == hipSuccess;
    for (int k = 0; ok && k < 4; k++) {  // the small grid a few times: the answer must not depend on where the dispatcher stood
      __atomic_store_n(c->dsync_status + 10, 0u, __ATOMIC_RELAXED);
      ok = launch_xcc_probe(c->dsync_status_dev + 10, kXcdBlocks, c->local_stream) == hipSuccess &&
           hipStreamSynchronize(c->local_stream) == hipSuccess;
      const uint32_t m = __atomic_load_n(c->dsync_status + 10, __ATOMIC_RELAXED);
      c->xcd_probe_mask = k == 0 ? m : (c->xcd_probe_mask & m);
    }
    if (ok) c->xcds = __builtin_popcount(__atomic_load_n(c->dsync_status + 8, __ATOMIC_RELAXED));
    (void)hipGetLastError();
    const bool covered = c->xcds > 0 && __builtin_popcount(c->xcd_probe_mask) >= c->xcds;
    if (c->body_sys < 0) c->body_sys = (c->xcds > 0 && !covered) ? 1 : 0;
    if (c->xcds > 0 && !covered)
      fprintf(stderr, "xmpi: rank %d: a %d-block grid reaches XCDs %#x of %d -- split collectives use system-scope loads / stores\n",
              c->rank, kXcdBlocks, c->xcd_probe_mask, (int)c->xcds);
  }
  if (c->body_sys < 0) c->body_sys = 0;
  // epochs of this communicator: above whatever earlier communicators left in ANY rank's (pooled, uncleared) page;
  // the same number on every rank.  It also tags the translations this communicator's kernels cache in the page.
  // (XMPI_TEST_EPOCH_BASE, tests: ... or above that many, as if the pages had seen them -- the counters' 32-bit edges in minutes)
  uint64_t base = (uint64_t)param_env("XMPI_TEST_EPOCH_BASE");
  for (int p = 0; p < N; p++) base = std::max(base, c->ctl->info(p)->flag_epoch);
  for (int p = 0; p < N; p++) c->p2p_out_seq[p] = seq0;
  c->dsync_epoch = base;
  c->dsync_base = base;
  c->dsync_tag = base + 1;
  c->dsync_ok = true;
  return XMPI_OK;
}

// The rank's helper thread (xmpi_init starts it for every job of more than one process):
//  * A rank must map what its peers register even while its own threads are blocked somewhere the library cannot see (a
//    hipStreamSynchronize of the caller's, a long computation): the helper looks once a millisecond -- one load per peer when
//    there is nothing to do.  (Every wait loop of the library looks as well, so inside the library the answer comes within
//    microseconds.)
//  * A peer whose PROCESS is gone is an error at once, with default settings (XMPI_TIMEOUT_S = 0: wait for ever): every
//    watchdog_ms (50) the helper asks the kernel whether the processes that joined as the other ranks still exist (pid + start
//    time, ctl.cpp peer_gone) and raises the job's abort flag for the first one that does not -- every host wait loop and every
//    waiting kernel (kdev.h spin_until, the LL and receive agents) polls that flag and comes back with XMPI_ERR_PEER.  What the
//    reference's peers get from their sockets (network.go:555,611,623: a lost connection fails Send / Receive immediately).
void dsync_start_helper(xmpi_comm* c) {
  if (c->size < 2 || c->dsync_helper.joinable()) return;
  bool other_process = false;
  for (int p = 0; p < c->size; p++) other_process = other_process || c->ctl->info(p)->pid != (int32_t)getpid();
  const bool watch = c->watchdog_ms > 0 && other_process;
  if (!c->dsync_ok && !watch) return;
  c->dsync_helper_stop = false;
  c->dsync_helper = std::thread([c, watch] {
    (void)hipSetDevice(c->device);
    const long every = std::max<long>(1, c->watchdog_ms);
    double next_look = now_seconds() + (double)every * 1e-3;
    while (!c->dsync_helper_stop.load(std::memory_order_acquire)) {
      dsync_service(c);
      if (watch && now_seconds() >= next_look) {
        if (!c->ctl->aborted()) (void)c->ctl->check_peers();
        next_look = now_seconds() + (double)every * 1e-3;
      }
      timespec ts{0, 1000000};
      nanosleep(&ts, nullptr);
    }
  });
}

void dsync_stop_helper(xmpi_comm* c) {
  if (c->dsync_helper.joinable()) {
    c->dsync_helper_stop.store(true, std::memory_order_release);
    c->dsync_helper.join();
  }
}

void dsync_finalize(xmpi_comm* c) {
  dsync_stop_helper(c);
  // the next user of the page starts above the last epoch written into it (graph replays are counted on the device:
  // the kernels copy the page's counter into the pinned status area)
  uint64_t last = c->dsync_epoch;
  if (c->ctl) last = std::max<uint64_t>(last, c->ctl->info(c->rank)->flag_epoch);  // (a communicator that never got going)
  if (c->dsync_status) last = std::max<uint64_t>(last, __atomic_load_n((const uint64_t*)(c->dsync_status + 2), __ATOMIC_ACQUIRE));
  // the flag self-test's token lies in the peers' (never cleared) pages whatever the vote said: the next communicator's token -- and
  // epochs -- start above it, or a stale token would pass a self-test no store arrived for
  last = std::max<uint64_t>(last, c->dsync_selftest_token);
  last += 1;  // every communicator gets a number of its own (dsync_tag = base + 1), also one that never ran a collective: the
              // tag marks its translation-cache entries and its Send / Receive message numbers in the (uncleared) page
  for (auto& p : c->dsync_prof_pending) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
  }
  c->dsync_prof_pending.clear();
  for (int p = 0; p < c->size; p++)
    if (c->peer_page_opened[p]) ipc_close_shared(c->peer_page[p]);
  if (c->host_bounce_dev) (void)hipHostFree(c->host_bounce);
  c->host_bounce = c->host_bounce_dev = nullptr;
  if (c->dsync_status) (void)hipHostFree(c->dsync_status);
  c->dsync_status = nullptr;
  if (c->v_rec) (void)hipHostFree(c->v_rec);
  c->v_rec = c->v_rec_dev = nullptr;
  if (c->dsync_res) (void)hipFree(c->dsync_res);
  c->dsync_res = nullptr;
  if (c->dsync_order_ev) (void)hipEventDestroy(c->dsync_order_ev);
  c->dsync_order_ev = nullptr;
  if (c->dsync_table) (void)hipHostFree(c->dsync_table);
  c->dsync_table = nullptr;
  for (auto& p : c->p2p_pending)
    for (void* b : p.bufs) (void)heap_free(b);
  c->p2p_pending.clear();
  for (auto& b : c->dsync_deferred) {
    (void)hipEventDestroy(b.done);
    for (void* p : b.bufs) (void)heap_free(p);
  }
  c->dsync_deferred.clear();
  for (void* p : c->dsync_leaked) (void)heap_free(p);
  c->dsync_leaked.clear();
  if (c->land_block) (void)heap_free(c->land_block);
  c->land_block = nullptr;
  c->land_block_bytes = 0;
  if (c->dpage) pool_release(c->dpage, last);
  c->dpage = nullptr;
  (void)hipGetLastError();
}

// Map what the peers have published since this rank last looked, and acknowledge.  Cheap when there is nothing
// to do (one load per peer); safe to call from any thread of the rank (a second caller just skips).
void dsync_service(xmpi_comm* c) {
  if (!c->dsync_ok) return;
  std::unique_lock<std::mutex> l(c->dsync_mu, std::try_to_lock);
  if (!l.owns_lock()) return;
  const int mypid = (int)getpid();
  for (int p = 0; p < c->size; p++) {
    if (p == c->rank) continue;
    PubTable* pt = c->ctl->published(p);
    const uint64_t n = pt->count.load(std::memory_order_acquire);
    uint64_t k = c->dsync_seen[p];
    if (k == n) continue;
    (void)hipSetDevice(c->device);  // may be the first HIP call of this thread (a wait loop of Send / Receive)
    for (; k < n; k++) {
      const PubEntry& e = pt->e[k % kPubRing];
      const int slot = (int)(e.reserved & 0xff);
      DsyncEntry ent;
      memset(&ent, 0, sizeof ent);
      ent.gen = e.gen;
      ent.bytes = e.bytes;
      if (c->ctl->info(p)->pid == mypid) {
        ent.base = e.base;  // same address space
      } else {
        BufRef ref;
        memset(&ref, 0, sizeof ref);
        ref.base = e.base;
        ref.gen = e.gen;
        ref.bytes = e.bytes;
        memcpy(ref.handle, e.handle, sizeof ref.handle);
        void* mapped = nullptr;
        if (zc_import(c, p, ref, &mapped)) ent.base = (uint64_t)(uintptr_t)mapped;
        else ent.gen = 0;  // cannot be mapped here: a kernel that meets it reports DSYNC_UNMAPPED
      }
      if (slot >= 0 && slot < kDsyncArenas) {  // the number last: a kernel that reads it (acquire) sees the rest
        DsyncEntry* t = &c->dsync_table[p * kDsyncArenas + slot];
        __atomic_store_n(&t->gen, 0, __ATOMIC_RELEASE);
        t->base = ent.base;
        t->bytes = ent.bytes;
        __atomic_store_n(&t->gen, ent.gen, __ATOMIC_RELEASE);
      }
    }
    c->dsync_seen[p] = n;
    c->ctl->acked(c->rank, p)->store(n, std::memory_order_release);
  }
}

}  // namespace xmpi
