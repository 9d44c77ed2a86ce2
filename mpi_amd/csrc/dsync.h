// dsync.h -- what the parts of the device-synchronised collectives share.  Host only, private to them:
//   dsync_plan.cpp   what a call is and what every rank launches for it (pure: route, signature, segments, grid)
//   dsync_call.cpp   the call lifecycle: publish / acks, lent blocks, the pinned bounce, waits, DsyncCall
//   dsync.cpp        one collective, start to end (dsync_collective, the LL form)
//   dsync_p2p.cpp    stream-ordered Send / Receive
//   vcoll.cpp        xmpi_alltoallv (its device form, dsync_alltoallv, is built from the same parts)
// The rest of the library sees the declarations in comm.h only.
#pragma once
#include <algorithm>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

// a collective's arguments, as its steps read them
struct CollArgs {
  int coll, root, dtype, op;
  size_t count, es;               // elements per rank (reduce-scatter, all-to-all: per block), bytes per element
  size_t unit;                    // count x es: the message, or -- reduce-scatter, all-to-all -- the block one rank gives one peer
  size_t send_bytes, recv_bytes;  // what the buffers hold (plan.h coll_send_bytes / coll_recv_bytes)
};

struct Resolved {
  const void* send = nullptr;
  void* recv = nullptr;
  BufRef sref, rref;
  void* tmp_send = nullptr;  // registered stand-ins of buffers the peers cannot map
  void* tmp_recv = nullptr;
};

struct DsyncRoute {
  enum Form { LL, FOLD, PUSH_ONLY, STEPPED } form = FOLD;  // FOLD: one kernel or meet / body / done (bcast and allgather: theirs)
  int algo = XMPI_ALGO_AUTO;        // the schedule as it runs: after the table and the capture demotions
  int sched_algo = XMPI_ALGO_AUTO;  // ... a stepped kernel by its pull form's name (RING, RHD, TREE)
  bool sched_push = false;          // ... and whether it pushes
  int split_pref = -1;              // one kernel (0) or meet / body / done (1); -1: by size (dsync_split_bytes)
  int unroll = 1;
  int refused = -1;                 // the rejected candidate (xmpi_comm::CAND_*) the caller named: nothing runs; -1: none
};

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

// the call signature the kernels announce and compare (DsyncArgs::sig)
inline uint64_t sig_mix(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x100000001B3ull;
  return h ^ (h >> 29);
}
inline uint64_t sig_fold(uint64_t h) { return std::max<uint64_t>(1, (h ^ (h >> 32)) & 0xffffffffull); }

// ---- dsync_plan.cpp.  Pure: from the communicator and the arguments only, the same answer on every rank
int dsync_grid(const xmpi_comm* c, size_t packets_per_segment, int nseg, int unroll);
DsyncRoute dsync_route(const xmpi_comm* c, int coll, int algo, size_t unit, bool capturing, bool wide = false);  // wide: a reduction of the fold family only (comm.h fold_only)
uint64_t call_sig(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt);
FoldPlan plan_for(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt);  // the fold family's plan of a call (not LL, not STEPPED)
size_t plan_sched(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt, const DsyncArgs& a, DsyncSchedArgs* out, int* gx_out);

// ---- dsync_call.cpp
int dsync_publish(xmpi_comm* c, const BufRef& ref, int* slot_out, uint64_t* pub_index, bool capturing = false);
int dsync_await_acks(xmpi_comm* c, uint64_t pub_index);
void* lend_standin(xmpi_comm* c, std::vector<void*>& lent, size_t bytes, BufRef* ref, int* rc);
int capture_needs_registered();  // sets the error text of a capture whose buffer would need a stand-in; XMPI_ERR_ARG
bool host_bounce_ready(xmpi_comm* c);
hipError_t bounce_copy(xmpi_comm* c, void* dst, const void* src, size_t bytes, int which, uint64_t* done, uint64_t done_value, hipStream_t s);

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
  const bool capturing;           // the stream is being captured into a graph: nothing may be lent, waited for or sampled

  // opens the call: stream 0 is the communicator's own; the peers are served and lent blocks the streams have passed taken back;
  // then `capturing` is asked of the stream
  DsyncCall(xmpi_comm* comm, hipStream_t s, bool b);
  void* lend(size_t bytes);
  void* own_block(size_t bytes);   // the communicator's landing block, grown to `bytes`
  int order_behind_last();         // the rank's kernels run one at a time: behind the stream of the previous one
  void begin();                    // behind order_behind_last, before the first launch: the call's number, whether it is sampled
  bool prof_events();
  void keep_prof();
  int fail(int rc);
  int enqueued(void* home, size_t bytes);
  int wait_and_finish(void* home, size_t bytes);
};

// ---- dsync.cpp
int dsync_announce(DsyncCall& call, const Resolved& r, int* sslot, int* rslot);
DsyncArgs meet_args(const xmpi_comm* c, const Resolved& r, int sslot, int rslot);

}  // namespace xmpi
