// dsync_plan.cpp -- what a device-synchronised call is and what every rank launches for it: whether the path takes the call at all,
// its route (LL lines, the fold, push-only, a stepped kernel; refused), the signature the kernels compare, the segments of every
// kernel of the fold family, the shape of a stepped kernel, the grid.
//
// Every rank must decide all of this alike, so it is decided from the communicator and the arguments only.  The rule of this file:
// it calls no HIP function, writes no member of the communicator and sets no error text -- `const xmpi_comm*` in, structs out.
// Who launches what is planned here: dsync.cpp (dsync_collective), vcoll.cpp (the grid of dsync_alltoallv).
#include <algorithm>
#include <cstring>

#include "dsync.h"
#include "sched_steps.h"

namespace xmpi {

bool dsync_usable(const xmpi_comm* c) { return c->dsync_ok && c->dsync && c->size > 1; }

// blocks a kernel of this rank may keep waiting at once: the kernels of all ranks on one GPU spin together, so with
// several ranks per GPU they must all be resident (half of its 8192 wave slots, 4 waves per block, shared)
static long dsync_block_cap(const xmpi_comm* c) {
  if (c->dsync_grid_cap > 0) return c->dsync_grid_cap;
  // (a rank alone on its GPU keeps to half of the chip too: while its blocks wait for a late peer the caller's other streams
  // still find wave slots -- scripts/overlap_probe.hip: a full-chip compute kernel next to a waiting 1024-block collective
  // runs 5 % slower, next to the meet / body / done form 1.5 %)
  // (Eight processes on one GPU, 64 instead of 128 blocks per rank: 6 % faster at 256 MiB on one box, 12 % slower on the next --
  // scripts/r03_tiles.sh; XMPI_DSYNC_GRID=256 per rank = every wave slot of the chip: the kernels wait for each other for ever.)
  return 1024 / std::max(1, c->dsync_sharers);
}

int dsync_grid(const xmpi_comm* c, size_t packets_per_segment, int nseg, int unroll) {
  long cap = std::max<long>(1, dsync_block_cap(c) / std::max(1, nseg));
  // several tiles per block: every block costs seven polling lanes on this rank's page and a ticket, which is what a
  // small collective spends its time on (8 processes, 1 MiB: 32 blocks per rank -> 84 us, see profiles/README.md)
  const size_t per_block = (size_t)256 * (size_t)std::max(1, unroll) * (size_t)std::max<long>(1, c->dsync_tiles);
  const size_t want = (packets_per_segment + per_block - 1) / per_block;
  return (int)std::max<size_t>(1, std::min<size_t>(want, (size_t)cap));
}

// which calls the device-synchronised path takes (the same answer on every rank: it depends on the job's layout
// and the arguments only)
bool dsync_takes(const xmpi_comm* c, int coll, int algo) {
  if (!dsync_usable(c)) return false;
  if (!c->windows_ok) return true;  // a job without windows has no staged step tables: DIRECT and whatever else names them is the fold
  switch (algo) {
    case XMPI_ALGO_AUTO: return c->zero_copy != 0;
    case XMPI_ALGO_ZCOPY:
    case XMPI_ALGO_ZPUSH:
    case XMPI_ALGO_LL: return true;
    case XMPI_ALGO_RING:  // the stepped kernels (sched.hip), pull and push form
    case XMPI_ALGO_RING_PUSH: return coll == COLL_ALLREDUCE || coll == COLL_ALLGATHER;
    case XMPI_ALGO_RHD:
    case XMPI_ALGO_RHD_PUSH: return coll == COLL_ALLREDUCE;
    case XMPI_ALGO_TREE:
    case XMPI_ALGO_TREE_PUSH: return coll == COLL_BCAST || coll == COLL_REDUCE;
    default: return false;
  }
}

// From the communicator and the arguments only -- the same answer on every rank, so every rank refuses alike, hands the same calls
// to LL and launches the same form.  Pure: no HIP, no counters, no error text.
// unit: the message -- reduce-scatter, all-to-all: the BLOCK, which is what a slot of LL lines has to hold and what every link carries
DsyncRoute dsync_route(const xmpi_comm* c, int coll, int algo, size_t unit, bool capturing, bool wide) {
  DsyncRoute rt;
  rt.unroll = (int)std::max<long>(1, std::min<long>(2, c->dsync_unroll));
  // the schedule: what the caller named, or the library's own table (xmpi_tune fills it; untuned: the zero-copy fold, split by size)
  if (algo == XMPI_ALGO_AUTO) {
    int cls = 0;
    while (cls + 1 < xmpi_comm::kTuneClasses && (unit >> (cls + 9)) != 0) cls++;
    if (c->tuned && coll >= 0 && coll < kTunedColls) {
      if (c->tune_algo[coll][cls] >= 0) algo = c->tune_algo[coll][cls];
      if (c->tune_split[coll][cls] >= 0) rt.split_pref = c->tune_split[coll][cls];
      if (c->tune_unroll[coll][cls] > 0) rt.unroll = c->tune_unroll[coll][cls];
      // XMPI_SUM_WIDE (f16 / bf16): a stepped schedule passes partial sums between ranks in the 16-bit type -- where the table names
      // one, the fold runs instead (as under capture below: by the arguments, so every rank decides alike).  A caller naming one
      // never gets here: api.cpp refuses.
      if (wide && algo_stepped(algo)) algo = XMPI_ALGO_ZCOPY;
    }
    // untuned: short messages go as {data, flag} lines (ll.hip) -- one one-way hop instead of two round trips
    if (algo == XMPI_ALGO_AUTO && c->zero_copy && unit <= (size_t)std::max<long>(0, c->ll_bytes)) algo = XMPI_ALGO_LL;
  }
  // A schedule whose ANSWERS xmpi_tune or xmpi_init's self-check found wrong on this machine (tune_rejected: the outcome of a vote,
  // the same bits on every rank) is not run for a caller: AUTO never leads here (the table leaves it out, apply_rejections the untuned
  // rules), so this is a caller -- or a table written by hand -- naming it.  Every rank refuses alike, before anything is lent,
  // announced or moved.
  const uint32_t rejected = (c->tune_running || coll < 0 || coll >= kTunedColls) ? 0u : c->tune_rejected[coll];
  auto no = [rejected](int cand) { return ((rejected >> cand) & 1u) != 0; };
  if (algo == XMPI_ALGO_LL) {
    if (unit <= kLLMaxPayload) {
      rt.form = DsyncRoute::LL;
      rt.algo = algo;
      if (no(xmpi_comm::CAND_LL)) rt.refused = xmpi_comm::CAND_LL;
      return rt;
    }
    algo = XMPI_ALGO_ZCOPY;  // named, but too long for the slots: the fold (the same decision on every rank)
  }
  // the push forms of the stepped kernels: the same schedule, the data stored into the peer instead of loaded from it
  rt.sched_push = algo == XMPI_ALGO_RING_PUSH || algo == XMPI_ALGO_RHD_PUSH || algo == XMPI_ALGO_TREE_PUSH;
  rt.sched_algo = algo == XMPI_ALGO_RING_PUSH ? XMPI_ALGO_RING : algo == XMPI_ALGO_RHD_PUSH ? XMPI_ALGO_RHD
                  : algo == XMPI_ALGO_TREE_PUSH ? XMPI_ALGO_TREE : algo;
  if (capturing) {
    // A graph cannot hold what is lent per call -- a landing block, the tree reduce's accumulator: replays would use it after it
    // went back to the arena.  Captured, a push form runs as its pull form (the same operands, order and association: the same
    // bits) and the tree reduce as the fold -- whatever named them, the caller or the tuner's table.  Every rank captures a
    // collective or none does (as with push-only below), so every rank decides alike: by the arguments, not by what IT would lend.
    if (rt.sched_push) algo = rt.sched_algo;
    rt.sched_push = false;
    if (rt.sched_algo == XMPI_ALGO_TREE && coll == COLL_REDUCE) algo = rt.sched_algo = XMPI_ALGO_ZCOPY;
  }
  rt.algo = algo;
  const int s = rt.sched_algo;
  if ((s == XMPI_ALGO_RING && (coll == COLL_ALLREDUCE || coll == COLL_ALLGATHER)) || (s == XMPI_ALGO_RHD && coll == COLL_ALLREDUCE) ||
      (s == XMPI_ALGO_TREE && (coll == COLL_BCAST || coll == COLL_REDUCE))) {
    rt.form = DsyncRoute::STEPPED;
    const int cand = s == XMPI_ALGO_RING ? (rt.sched_push ? xmpi_comm::CAND_RING_PUSH : xmpi_comm::CAND_RING)
                     : s == XMPI_ALGO_RHD ? (rt.sched_push ? xmpi_comm::CAND_RHD_PUSH : xmpi_comm::CAND_RHD)
                                          : (rt.sched_push ? xmpi_comm::CAND_TREE_PUSH : xmpi_comm::CAND_TREE);
    if (no(cand)) rt.refused = cand;
  } else if (algo == XMPI_ALGO_ZPUSH && (coll == COLL_ALLREDUCE || coll == COLL_REDUCE || coll == COLL_REDUCE_SCATTER) && !capturing) {
    // (under capture the push-only form is the fold: its staging area is a block the communicator may replace later)
    rt.form = DsyncRoute::PUSH_ONLY;
    if (no(xmpi_comm::CAND_ZPUSH)) rt.refused = xmpi_comm::CAND_ZPUSH;
  } else if (coll == COLL_BCAST) {  // (its fold is one kernel whatever the size)
    if (no(xmpi_comm::CAND_FOLD)) rt.refused = xmpi_comm::CAND_FOLD;
  } else {
    // one kernel or meet / body / done is each rank's own choice (the two mix: dsync_begin / the meet kernel speak one protocol):
    // a rank keeps to the one of the two that is right here
    if (no(xmpi_comm::CAND_FOLD) && no(xmpi_comm::CAND_SPLIT)) rt.refused = xmpi_comm::CAND_FOLD;
    else if (no(xmpi_comm::CAND_SPLIT)) rt.split_pref = 0;
    else if (no(xmpi_comm::CAND_FOLD) && c->dsync_res) rt.split_pref = 1;
  }
  return rt;
}

namespace {

// bcast: the root stores into every buffer itself -- two ranks, or up to zc_bcast_push_bytes -- or scatters, and every rank forwards
bool bcast_forwards(const xmpi_comm* c, size_t bytes) { return c->size > 2 && bytes > (size_t)std::max<long>(0, c->zc_bcast_push_bytes); }

uint32_t everyone(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }

// allreduce / reduce: every rank folds its chunk of everybody's send buffer, in rank order, into everybody's receive buffer (reduce:
// the root's)
FoldPlan plan_fold(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size;
  size_t off = 0, cnt = 0;
  zc_chunk(k.count, k.es, N, c->rank, &off, &cnt);
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = cnt > 0 ? 1 : 0;
  s.seg[0].src_off = s.seg[0].dst_off = off * k.es;
  s.seg[0].count = cnt;
  s.seg[0].src_mask = everyone(N);
  s.seg[0].dst_mask = k.coll == COLL_REDUCE ? (1u << k.root) : everyone(N);
  s.nsrc = N;
  s.dtype = k.dtype;
  s.op = k.op;
  s.packets = cnt / std::max<size_t>(1, 16 / k.es);
  s.moved = (size_t)(N + (k.coll == COLL_REDUCE ? 1 : N)) * cnt * k.es;
  s.split_pref = split_pref;
  return p;
}

// allgather: every rank stores its block into its place in everybody's receive buffer
FoldPlan plan_allgather(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = 1;
  s.seg[0].dst_off = (size_t)c->rank * k.send_bytes;
  s.seg[0].count = k.send_bytes;
  s.seg[0].src_mask = 1u << c->rank;
  s.seg[0].dst_mask = everyone(c->size);
  s.packets = k.send_bytes / 16;
  s.moved = (size_t)(1 + c->size) * k.send_bytes;
  s.split_pref = split_pref;
  return p;
}

// reduce-scatter: the allreduce's fold with one local destination -- every rank folds block `me` of everybody's send buffer, in rank
// order, into its own receive buffer.  Block `me` starts at me x B, which unlike a zc_chunk cut need not be 16-byte aligned:
// blocks that are a multiple of 16 bytes take the kernel's packet path, others its one-element-per-lane path (correct, slow).
FoldPlan plan_reduce_scatter(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size;
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = 1;
  s.seg[0].src_off = (size_t)c->rank * k.unit;
  s.seg[0].dst_off = 0;
  s.seg[0].count = k.count;
  s.seg[0].src_mask = everyone(N);
  s.seg[0].dst_mask = 1u << c->rank;
  s.nsrc = N;
  s.dtype = k.dtype;
  s.op = k.op;
  s.packets = k.count / std::max<size_t>(1, 16 / k.es);
  s.moved = (size_t)(N + 1) * k.unit;
  s.split_pref = split_pref;
  return p;
}

// all-to-all, push form: one segment per destination j -- my block j into place `me` of rank j's receive buffer (the own block
// is a segment like the others).  Every payload byte crosses its link as a posted store; N <= kDsyncRanks segments fit.
FoldPlan plan_alltoall(const xmpi_comm* c, const CollArgs& k, int split_pref) {
  const int N = c->size, me = c->rank;
  FoldPlan p;
  FoldStep& s = p.k[0];
  for (int d = 0; d < N; d++) {  // (own block first, then the next rank's: the ranks do not all store into rank 0 first)
    const int j = (me + d) % N;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = (size_t)j * k.unit;
    g.dst_off = (size_t)me * k.unit;
    g.count = k.unit;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << j;
  }
  s.packets = k.unit / 16;
  s.moved = 2 * (size_t)N * k.unit;
  s.split_pref = split_pref;
  return p;
}

// reduce-scatter, push-only (XMPI_ALGO_ZPUSH): plan_push_only below with blocks for zc_chunk's cuts -- my block q into region `me`
// of rank q's landing block, then a local fold in rank order into the receive buffer.
FoldPlan plan_reduce_scatter_push(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  const size_t region = (k.unit + 255) / 256 * 256;
  FoldPlan p;
  p.kernels = 2;
  p.land = region * (size_t)N;
  FoldStep& s = p.k[0];
  for (int d = 1; d < N; d++) {
    const int q = (me + d) % N;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = (size_t)q * k.unit;
    g.dst_off = (size_t)me * region;
    g.count = k.unit;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << q;
    g.dst_to_land = 1;
  }
  s.packets = k.unit / 16;
  s.moved = 2 * (size_t)(N - 1) * k.unit;
  p.k[1] = plan_reduce_scatter(c, k, -1).k[0];
  p.k[1].seg[0].src_from_recv = 2;
  p.k[1].seg[0].stage_stride = region;
  return p;
}

// bcast (`send` and `recv` are the same buffer on every rank), the root pushes: it stores into every buffer, the others only take
// part in the rendezvous.  (The ranks differ in what they launch: the one-kernel form, whose shape does not matter.)
FoldPlan plan_bcast_push(const xmpi_comm* c, const CollArgs& k) {
  FoldPlan p;
  FoldStep& s = p.k[0];
  s.nseg = c->rank == k.root ? 1 : 0;
  s.seg[0].count = k.send_bytes;
  s.seg[0].src_mask = 1u << k.root;
  s.seg[0].dst_mask = everyone(c->size) & ~(1u << k.root);
  s.packets = k.send_bytes / 16;
  s.moved = c->rank == k.root ? (size_t)c->size * k.send_bytes : 0;
  return p;
}

// bcast, scatter + forward: the root scatters chunk j to rank j (one segment per destination, each over its own link), then every
// rank forwards its chunk to the others: each link carries S/N twice instead of the root's links carrying S
FoldPlan plan_bcast_forward(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  FoldPlan p;
  p.kernels = 2;
  FoldStep& s = p.k[0];
  if (me == k.root) {
    for (int j = 0; j < N; j++) {
      size_t off = 0, cnt = 0;
      zc_chunk(k.count, k.es, N, j, &off, &cnt);
      if (j == k.root || cnt == 0) continue;
      DsyncSeg& g = s.seg[s.nseg++];
      g.src_off = g.dst_off = off * k.es;
      g.count = cnt * k.es;
      g.src_mask = 1u << k.root;
      g.dst_mask = 1u << j;
      s.packets = std::max(s.packets, cnt * k.es / 16);
      s.moved += 2 * cnt * k.es;
    }
  }
  size_t off = 0, cnt = 0;
  zc_chunk(k.count, k.es, N, me, &off, &cnt);
  FoldStep& f = p.k[1];
  f.nseg = cnt > 0 ? 1 : 0;
  f.seg[0].src_off = f.seg[0].dst_off = off * k.es;
  f.seg[0].count = cnt * k.es;
  f.seg[0].src_mask = 1u << me;
  f.seg[0].dst_mask = everyone(N) & ~(1u << me) & ~(1u << k.root);
  f.packets = cnt * k.es / 16;
  f.moved = (size_t)(N - 1) * cnt * k.es;
  return p;
}

// Push-only (XMPI_ALGO_ZPUSH): the fold with nothing READ over xGMI -- loads over a link are round trips, stores are posted.
// Two device-synchronised kernels: every rank stores its contribution to chunk q into region `me` of rank q's own block
// (DsyncCall::own_block: the communicator's staging area, announced with the buffers; chunks cut as the fold cuts them, zc_chunk
// -- so in place and ragged counts work like anything else); then, all of chunk `me` being local, folds it in rank order and
// stores the result into its place in everybody's receive buffer.  One hop each way, S / N per link direction and kernel.
FoldPlan plan_push_only(const xmpi_comm* c, const CollArgs& k) {
  const int N = c->size, me = c->rank;
  size_t maxc = 0;
  for (int q = 0; q < N; q++) {
    size_t off = 0, cnt = 0;
    zc_chunk(k.count, k.es, N, q, &off, &cnt);
    maxc = std::max(maxc, cnt * k.es);
  }
  const size_t region = (maxc + 255) / 256 * 256;
  FoldPlan p;
  p.kernels = 2;
  p.land = region * (size_t)N;
  FoldStep& s = p.k[0];
  for (int q = 0; q < N; q++) {
    size_t off = 0, cnt = 0;
    zc_chunk(k.count, k.es, N, q, &off, &cnt);
    if (q == me || cnt == 0) continue;
    DsyncSeg& g = s.seg[s.nseg++];
    g.src_off = off * k.es;           // my contribution to chunk q ...
    g.dst_off = (size_t)me * region;  // ... into region `me` of rank q's block
    g.count = cnt * k.es;
    g.src_mask = 1u << me;
    g.dst_mask = 1u << q;
    g.dst_to_land = 1;
    s.packets = std::max(s.packets, cnt * k.es / 16);
    s.moved += 2 * cnt * k.es;
  }
  // every contribution to chunk `me` is local now (the first kernel's close: every peer's stores have landed): ONE more kernel
  // folds them in rank order and stores the result into its place in everybody's receive buffer -- the fold's own kernels
  // (one kernel, or meet / body / done by size) with local sources.  Its rendezvous doubles as "my buffers may be written";
  // nobody's block is written again before its owner's next collective has announced it.
  p.k[1] = plan_fold(c, k, -1).k[0];
  p.k[1].seg[0].src_from_recv = 2;
  p.k[1].seg[0].stage_stride = region;
  return p;
}

}  // namespace

// What this call is, for the peers to compare with theirs (kdev.h dsync_begin): ranks that are not in the same collective, on the
// same schedule, over the same bytes end with an error before any of them has touched another's memory -- instead of a hang, or
// of a fold over buffers of different lengths.  (One kernel or meet / body / done is NOT part of it: those mix.)
uint64_t call_sig(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt) {
  const bool reduces = coll_reduces(k.coll), rooted = k.coll == COLL_BCAST || k.coll == COLL_REDUCE;
  const uint64_t form = rt.form == DsyncRoute::STEPPED ? 16u + 2u * (uint64_t)rt.sched_algo + (rt.sched_push ? 1u : 0u)
                        : rt.form == DsyncRoute::PUSH_ONLY ? 2u
                        : (k.coll == COLL_BCAST && bcast_forwards(c, k.send_bytes)) ? 3u : 1u;
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (uint64_t v : {(uint64_t)k.coll + 1, form, (uint64_t)k.send_bytes, reduces ? (uint64_t)k.dtype + 1 : 0, reduces ? (uint64_t)k.op + 1 : 0,
                     rooted ? (uint64_t)k.root + 1 : 0})
    h = sig_mix(h, v);
  return sig_fold(h);
}

// the fold family's plan of a call: by the route's form, then by the collective
FoldPlan plan_for(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt) {
  const int coll = k.coll;
  return rt.form == DsyncRoute::PUSH_ONLY        ? (coll == COLL_REDUCE_SCATTER ? plan_reduce_scatter_push(c, k) : plan_push_only(c, k))
         : coll == COLL_REDUCE_SCATTER           ? plan_reduce_scatter(c, k, rt.split_pref)
         : coll == COLL_ALLTOALL                 ? plan_alltoall(c, k, rt.split_pref)
         : coll == COLL_ALLGATHER                ? plan_allgather(c, k, rt.split_pref)
         : coll != COLL_BCAST                    ? plan_fold(c, k, rt.split_pref)
         : bcast_forwards(c, k.send_bytes)       ? plan_bcast_forward(c, k)
                                                 : plan_bcast_push(c, k);
}

// ring / recursive halving + doubling / binary tree: ONE kernel per rank runs every step of the schedule, the steps released by
// flag words between the peers' kernels (sched.hip) -- the schedules north_star names, without a host between their steps.
// The kernel's arguments and shape (channels, *gx workers per channel, pieces, orders: part of the signature); returns the
// traffic figure.
size_t plan_sched(const xmpi_comm* c, const CollArgs& k, const DsyncRoute& rt, const DsyncArgs& a, DsyncSchedArgs* out, int* gx_out) {
  const int N = c->size, me = c->rank, coll = k.coll;
  const size_t send_bytes = k.send_bytes;
  const bool push = rt.sched_push;
  DsyncSchedArgs& sa = *out;
  memset(&sa, 0, sizeof sa);
  sa.d = a;
  sa.root = k.root;
  sa.count = k.count;
  sa.elem_size = (uint32_t)k.es;
  sa.pieces = 1;
  sa.push = push ? 1u : 0u;
  size_t step_bytes = send_bytes, traffic = 0;  // what the largest step of the schedule moves
  int nchan = 1;
  if (rt.sched_algo == XMPI_ALGO_RING) {
    sa.sched = coll == COLL_ALLREDUCE ? SCHED_RING_ALLREDUCE : SCHED_RING_ALLGATHER;
    step_bytes = coll == COLL_ALLREDUCE ? (send_bytes + (size_t)N - 1) / (size_t)N : send_bytes;
    // every channel is a different cyclic order of the ranks (plan.cpp ring_order: on an even mesh N-2 directed rings
    // that share no link direction); ranks sharing a GPU have no links to spread over
    const int avail = std::min(ring_channel_count(N), kMaxSchedChannels);
    // (the shape of a stepped kernel -- channels, workers -- is protocol: worker w waits for worker w of its peer.  It follows
    // the job's most crowded GPU, which every rank reads alike, not this rank's own: 5 ranks on 2 GPUs sit 3 + 2)
    nchan = c->sched_channels > 0 ? (int)std::min<long>(c->sched_channels, avail) : (c->dsync_sharers_job > 1 ? 1 : avail);
    // (reduce-scatter 2 reads + 1 write per step, allgather 1 + 1; the push form reads its own first chunk once more)
    traffic = coll == COLL_ALLREDUCE ? (5 * (size_t)(N - 1) + (push ? 1 : 0)) * step_bytes : 2 * (size_t)N * send_bytes;
  } else if (rt.sched_algo == XMPI_ALGO_RHD) {
    sa.sched = SCHED_RHD_ALLREDUCE;
    step_bytes = send_bytes / 2;
    // halving: 3 x (S/2 + S/4 + ...), doubling: 2 x the same; push form: the landing regions are written and read -- one more
    traffic = (push ? 6 : 5) * (send_bytes - send_bytes / (size_t)N);
    if ((N & (N - 1)) != 0) traffic += 3 * send_bytes;     // (no power of two: the fold-in / fold-out steps, at most)
  } else {
    sa.sched = coll == COLL_BCAST ? SCHED_TREE_BCAST : SCHED_TREE_REDUCE;
    const size_t piece = (size_t)std::max<long>(4096, c->tree_piece_bytes);
    sa.pieces = (int)std::min<size_t>(32, std::max<size_t>(1, (send_bytes + piece - 1) / piece));
    step_bytes = (send_bytes + (size_t)sa.pieces - 1) / (size_t)sa.pieces;
    const int v = (me - k.root + N) % N;
    const size_t children = (size_t)((2 * v + 1 < N) + (2 * v + 2 < N));
    if (coll == COLL_BCAST) {  // pull: a node reads its parent's piece and writes its own; push: it reads its own and writes each child's
      traffic = push ? 2 * send_bytes * children : (me == k.root ? 0 : 2 * send_bytes);
    } else {  // pull: 2 reads + 1 write per child; push: own input + one slot per child read, one buffer stored (upwards, or the result)
      traffic = push ? (children + 2) * send_bytes : 3 * send_bytes * children;
    }
  }
  const size_t tiles = std::max<size_t>(1, (step_bytes + kSchedTileBytes - 1) / kSchedTileBytes);
  const long job_cap = c->dsync_grid_cap > 0 ? c->dsync_grid_cap : 1024 / std::max(1, c->dsync_sharers_job);
  long workers = c->sched_grid > 0 ? c->sched_grid : (long)std::min<size_t>(tiles, (size_t)job_cap);
  workers = std::max<long>(1, std::min<long>(workers, kStepSlots));
  nchan = (int)std::max<long>(1, std::min<long>(nchan, workers));
  const int gx = (int)std::max<long>(1, workers / nchan);
  sa.nchan = nchan;
  // (worker w of a rank waits for worker w of its peer, over the same channels and pieces: the shape is part of the call)
  sa.d.sig = sig_fold(sig_mix(sig_mix(sig_mix(a.sig, (uint64_t)nchan), (uint64_t)gx), (uint64_t)sa.pieces));
  for (int ch = 0; ch < nchan; ch++) {
    std::vector<int> ord;
    ring_order(N, ch, &ord);
    for (int i = 0; i < N; i++) sa.order[ch][i] = (uint8_t)ord[(size_t)i];
  }
  *gx_out = gx;
  return traffic;
}

}  // namespace xmpi
