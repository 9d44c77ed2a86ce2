// tune.cpp -- the library checks and times its schedules on the machine it runs on: xmpi_init's self-check, xmpi_tune.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "comm.h"
#include "kernels.h"

namespace xmpi {

// ---- the library checks its schedules' ANSWERS on the machine it runs on ------------------------------------------------------
// The reference's own benchmark verifies every echo before it reports a time (examples/bounce/bounce.go:103-112,131-136), its
// handshake checks what came back (network.go:343-351).  Here: whoever times a schedule (xmpi_tune) or is about to rely on one
// untuned (xmpi_init's self-check) first runs it ONCE on patterned inputs -- rank r's send buffer = the counter-based pattern with
// seed kCheckSeed + r (kernels.hip fill_kernel, pattern 3: signed multiples of 2^-12 below 4 in magnitude: the float32 sum of
// sixteen of them is exact in EVERY association, so every schedule must produce the same bits) --, compares the receive buffer with
// the result computed locally (N fills folded with the two-operand kernel: no communication), and votes through the control block.
constexpr size_t kSecondPassBytes = (size_t)1 << 20;  // per rank: eight ranks' buffers of that size sit in the L2s (8 x 4 MiB) together from one run to the next
constexpr long kTuneTimeoutS = 20;  // no-progress limit of a candidate run in a job that otherwise waits for ever
constexpr uint64_t kCheckSeed = 0x7A11D;
constexpr int kCheckPattern = 3;

static void append(std::string& why, const std::string& text) { why += (why.empty() ? "" : "; ") + text; }

// what the self-check (`at` = "") and the tuner ("first at ") say of a candidate whose answer differs
static std::string wrong_answers(int coll, int k, const char* at, size_t per_rank, uint64_t nbad) {
  char t[200];
  snprintf(t, sizeof t, "%s: %s gives wrong answers on this machine (%s%zu B per rank: %llu bytes differ on the worst rank)", coll_name(coll), xmpi_comm::kCandName[k],
           at, per_rank, (unsigned long long)nbad);
  return t;
}

// A candidate that HANGS on this machine (flag words that never arrive over a link, say) must not hang the job that merely asked
// which schedule is fastest: with the default "wait for ever" every wait of a candidate run -- host loops and waiting kernels -- has
// a no-progress limit of its own while one of these lives.
struct TuneTimeout {
  xmpi_comm* c;
  const long keep;
  explicit TuneTimeout(xmpi_comm* comm) : c(comm), keep(comm->timeout_s) {
    if (keep == 0) c->timeout_s = kTuneTimeoutS;
  }
  ~TuneTimeout() { c->timeout_s = keep; }
};

int job_barrier(xmpi_comm* c) {
  dsync_service(c);
  Backoff bo;
  arm(bo, c);
  return c->ctl->barrier(wait_limit(c), &bo);
}

// every rank publishes a row, all meet, everybody reads the same maxima
static int vote_max(xmpi_comm* c, const double* us, const uint64_t* bad, int n, double* us_max, uint64_t* bad_max) {
  TuneVote* mine = c->ctl->vote(c->rank);
  for (int k = 0; k < kTuneCands; k++) {
    mine->us[k] = (us && k < n) ? us[k] : 0.0;
    mine->bad[k] = (bad && k < n) ? bad[k] : 0;
  }
  int rc = job_barrier(c);
  if (rc != XMPI_OK) return rc;
  for (int k = 0; k < n; k++) {
    double u = 0;
    uint64_t b = 0;
    for (int p = 0; p < c->size; p++) {
      const TuneVote* v = c->ctl->vote(p);
      u = std::max(u, v->us[k]);
      b = std::max(b, v->bad[k]);
    }
    if (us_max) us_max[k] = u;
    if (bad_max) bad_max[k] = b;
  }
  return job_barrier(c);  // nobody writes its next row before everybody has read this one
}

struct AnswerCheck {
  xmpi_comm* c = nullptr;
  char *send = nullptr, *recv = nullptr, *expect = nullptr, *expect2 = nullptr;
  size_t cap = 0, cap2 = 0;  // bytes of each (expect2: the second pass is for messages a cache could still hold)
  int have_coll = -1;      // what `expect` holds
  size_t have_bytes = 0;
  double spent_s = 0;
  uint64_t* host_word = nullptr;      // pinned: where a count reaches the host without a device-to-host copy (kernels.hip word_to_host_kernel)
  uint64_t* host_word_dev = nullptr;
  bool twice = true;       // the caller's say on the second pass (xmpi_tune: every other size class)
  struct Spent {  // the time a method takes goes into spent_s, however it returns
    double& sum;
    const double t0 = now_seconds();
    ~Spent() { sum += now_seconds() - t0; }
  };

  int open(xmpi_comm* comm, size_t max_bytes) {
    c = comm;
    cap = max_bytes;
    send = (char*)heap_alloc(c->device, cap);
    recv = (char*)heap_alloc(c->device, cap);
    // (the expected results are this rank's own business: plain device memory -- a block of a registered arena is exported and mapped
    // by every peer, and four 256 MiB blocks per rank grew the arenas by a GiB each: 8 .. 33 s of mapping on a fresh box)
    cap2 = std::min(cap, kSecondPassBytes * (size_t)c->size);
    if (hipMalloc((void**)&expect, cap) != hipSuccess) expect = nullptr;
    if (hipMalloc((void**)&expect2, cap2) != hipSuccess) expect2 = nullptr;
    pinned_words(64, &host_word, &host_word_dev);
    if (!send || !recv || !expect || !expect2 || !host_word_dev) {
      close();
      set_last_error("xmpi_tune: out of device memory");
      return XMPI_ERR_NOMEM;
    }
    XMPI_HIP(launch_fill(send, cap / 4, XMPI_F32, kCheckPattern, kCheckSeed + (uint64_t)c->rank, c->local_stream));
    XMPI_HIP(hipStreamSynchronize(c->local_stream));
    return XMPI_OK;
  }
  void close() {
    if (c) {
      (void)hipStreamSynchronize(c->local_stream);
      (void)hipGetLastError();
    }
    if (send) (void)heap_free(send);
    if (recv) (void)heap_free(recv);
    if (expect) (void)hipFree(expect);
    if (expect2) (void)hipFree(expect2);
    if (host_word) (void)hipHostFree(host_word);
    host_word = host_word_dev = nullptr;
    (void)hipGetLastError();
    send = recv = expect = expect2 = nullptr;
  }
  size_t recv_bytes(int coll, size_t per_rank) const { return coll_recv_bytes(coll, c->size, per_rank); }
  // `expect` = what `coll` over `per_rank` bytes per rank (root 0) must leave in the receive buffer.  The pattern is a function of
  // the element's index: a shorter message is a prefix of a longer one's, so the sum and the broadcast are computed once, at `cap`.
  int expect_for(int coll, size_t per_rank) {
    Spent timer{spent_s};
    hipStream_t s = c->local_stream;
    const bool sum = coll == COLL_ALLREDUCE || coll == COLL_REDUCE;
    if (sum && !(have_coll == COLL_ALLREDUCE || have_coll == COLL_REDUCE)) {
      XMPI_HIP(launch_fill(expect, cap / 4, XMPI_F32, kCheckPattern, kCheckSeed, s));
      for (int r = 1; r < c->size; r++) {  // (the receive buffer is free between two candidates: the other ranks' inputs pass through it)
        XMPI_HIP(launch_fill(recv, cap / 4, XMPI_F32, kCheckPattern, kCheckSeed + (uint64_t)r, s));
        XMPI_HIP(launch_reduce2(expect, expect, recv, cap / 4, XMPI_F32, XMPI_SUM, s));
      }
    } else if (coll == COLL_ALLGATHER && !(have_coll == coll && have_bytes == per_rank)) {
      for (int r = 0; r < c->size; r++)
        XMPI_HIP(launch_fill(expect + (size_t)r * per_rank, per_rank / 4, XMPI_F32, kCheckPattern, kCheckSeed + (uint64_t)r, s));
    } else if (coll == COLL_BCAST && have_coll != coll) {
      XMPI_HIP(launch_fill(expect, cap / 4, XMPI_F32, kCheckPattern, kCheckSeed, s));
      if (c->rank == 0) XMPI_HIP(launch_fill(recv, cap / 4, XMPI_F32, kCheckPattern, kCheckSeed, s));  // the root's buffer IS the message
    }
    have_coll = coll;
    have_bytes = per_rank;
    return XMPI_OK;
  }
  // before the checked run: whatever an earlier candidate left in the receive buffer must not pass for this one's answer
  int arm(int coll, size_t per_rank) {
    Spent timer{spent_s};
    // (bcast: the root's buffer is the input; reduce: only the root's is written)
    const bool untouched = (coll == COLL_BCAST && c->rank == 0) || (coll == COLL_REDUCE && c->rank != 0);
    // (a kernel of the library's own on the rank's stream -- the constant 166.0, which no sum of sixteen pattern values can be --, not
    // hipMemsetAsync: the runtime's fills do not run on the stream's queue alone, see count_to_host)
    if (!untouched) XMPI_HIP(launch_fill(recv, recv_bytes(coll, per_rank) / 4, XMPI_F32, /*pattern=*/2, /*seed=*/165, c->local_stream));
    return XMPI_OK;
  }
  // The SECOND pass: the inputs change IN PLACE between two runs (every rank's buffer := 2 x itself, one local kernel; the expected
  // result doubles with it, exactly) -- what a caller's buffers do from one step to the next.  A reader that still holds lines of a
  // peer's buffer from the run before -- an L2 the schedule's acquire did not reach: the split form's once-per-XCD acquire is
  // exactly that bet -- folds OLD data, and only a changed input shows it: the first run of a fresh buffer never can.  For messages a
  // cache could still hold whole (kSecondPassBytes per rank); afterwards the inputs are what they were (refilled).
  bool second_pass(int coll, size_t per_rank) const {
    static const bool on = env_long("XMPI_CHECK_PASSES", 2) >= 2;  // (1: the first pass only -- A/B of what the second one costs)
    return on && per_rank <= kSecondPassBytes && recv_bytes(coll, per_rank) <= cap2;
  }
  int change_inputs(int coll, size_t per_rank) {
    Spent timer{spent_s};
    hipStream_t s = c->local_stream;
    if (coll != COLL_BCAST) XMPI_HIP(launch_reduce2(send, send, send, per_rank / 4, XMPI_F32, XMPI_SUM, s));
    else if (c->rank == 0) XMPI_HIP(launch_reduce2(recv, recv, recv, per_rank / 4, XMPI_F32, XMPI_SUM, s));
    XMPI_HIP(launch_reduce2(expect2, expect, expect, recv_bytes(coll, per_rank) / 4, XMPI_F32, XMPI_SUM, s));
    return XMPI_OK;
  }
  int restore_inputs(int coll, size_t per_rank) {
    Spent timer{spent_s};
    hipStream_t s = c->local_stream;
    if (coll != COLL_BCAST) XMPI_HIP(launch_fill(send, per_rank / 4, XMPI_F32, kCheckPattern, kCheckSeed + (uint64_t)c->rank, s));
    else if (c->rank == 0) XMPI_HIP(launch_fill(recv, per_rank / 4, XMPI_F32, kCheckPattern, kCheckSeed, s));
    return XMPI_OK;
  }
  // c->dev_words[0] -> *out, behind everything on the stream; no copy engine involved
  hipError_t count_to_host(uint64_t* out) {
    hipStream_t s = c->local_stream;
    __atomic_store_n(host_word, ~0ull, __ATOMIC_RELAXED);
    hipError_t e = launch_word_to_host(host_word_dev, c->dev_words, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    *out = __atomic_load_n(host_word, __ATOMIC_ACQUIRE);
    return e;
  }
  int verdict(int coll, size_t per_rank, uint64_t* bad, bool second = false) {
    *bad = 0;
    if (coll == COLL_REDUCE && c->rank != 0) return XMPI_OK;
    Spent timer{spent_s};
    hipStream_t s = c->local_stream;
    XMPI_HIP(launch_signal(c->dev_words, 0, s));
    XMPI_HIP(launch_count_mismatch(recv, second ? expect2 : expect, recv_bytes(coll, per_rank), c->dev_words, s));
    XMPI_HIP(count_to_host(bad));
    return XMPI_OK;
  }
};

struct TuneCand {
  int algo, split, unroll;
};
static std::vector<TuneCand> tune_candidates(const xmpi_comm* c) {
  const int u0 = (int)std::max<long>(1, std::min<long>(2, c->dsync_unroll));
  // the default comes first (xmpi_tune_decide keeps it on a tie); the order is xmpi_comm::CAND_*
  return {{XMPI_ALGO_ZCOPY, 0, u0},      {XMPI_ALGO_ZCOPY, 0, 3 - u0}, {XMPI_ALGO_ZCOPY, 1, u0},    {XMPI_ALGO_ZPUSH, 0, u0},
          {XMPI_ALGO_RING, 0, u0},       {XMPI_ALGO_RHD, 0, u0},       {XMPI_ALGO_LL, 0, u0},
          // the push forms of the stepped kernels (sched_steps.h): the same schedules with every payload byte STORED over its link
          // instead of loaded -- which of the two a link moves faster is the machine's to say
          {XMPI_ALGO_RING_PUSH, 0, u0},  {XMPI_ALGO_RHD_PUSH, 0, u0},
          // bcast and reduce: the tree kernels in both forms against the fold's two halves
          {XMPI_ALGO_TREE, 0, u0},       {XMPI_ALGO_TREE_PUSH, 0, u0}};
}
static void set_row(xmpi_comm* c, int coll, int cls, const TuneCand& cd) {  // a row of the table AUTO follows
  c->tune_algo[coll][cls] = (int8_t)cd.algo;
  c->tune_split[coll][cls] = (int8_t)cd.split;
  c->tune_unroll[coll][cls] = (int8_t)cd.unroll;
}
// which candidates a collective has: (the fold, LL lines) all four; allreduce every form of the fold and ring / halving in both
// forms; allgather the ring; bcast the tree (its fold is one kernel whatever the size); reduce what allreduce has of the fold, and
// the tree
static bool tune_offered(const xmpi_comm* c, int coll, const TuneCand& cd) {
  const int u0 = (int)std::max<long>(1, std::min<long>(2, c->dsync_unroll));
  const bool tree = cd.algo == XMPI_ALGO_TREE || cd.algo == XMPI_ALGO_TREE_PUSH;
  const bool ring = cd.algo == XMPI_ALGO_RING || cd.algo == XMPI_ALGO_RING_PUSH;
  const bool rhd = cd.algo == XMPI_ALGO_RHD || cd.algo == XMPI_ALGO_RHD_PUSH;
  switch (coll) {
    case COLL_ALLREDUCE: return !tree;
    case COLL_ALLGATHER: return !tree && !rhd && cd.algo != XMPI_ALGO_ZPUSH && cd.unroll == u0;
    case COLL_BCAST: return !ring && !rhd && cd.algo != XMPI_ALGO_ZPUSH && cd.unroll == u0 && cd.split == 0;
    default: return !ring && !rhd && cd.unroll == u0;  // COLL_REDUCE
  }
}

// Candidates `ks` of `coll` at `per_rank` bytes per rank: each runs once CHECKED (check: the warm-up that also maps whatever is
// new), then `iters` times against the clock.  us[k]: mean microseconds (min with what it held when keep_min); bad[k]: bytes of
// this rank's receive buffer that differ from the expected result.  Collective: every rank passes the same arguments.
static int tune_measure(xmpi_comm* c, AnswerCheck& chk, const std::vector<TuneCand>& cands, int coll, size_t per_rank, const std::vector<int>& ks,
                        int iters, bool check, bool keep_min, double* us, uint64_t* bad) {
  const long keep_split = c->dsync_split_bytes, keep_unroll = c->dsync_unroll;
  TuneTimeout limit(c);  // (until after the loop; the error names the candidate: leave it out with tune_mask, or set XMPI_TIMEOUT_S)
  int rc = XMPI_OK;
  for (size_t j = 0; j < ks.size() && rc == XMPI_OK; j++) {
    const int k = ks[j];
    const TuneCand& cd = cands[(size_t)k];
    rc = job_barrier(c);  // (everybody has left the previous candidate: its receive buffer is this rank's again)
    if (rc != XMPI_OK) break;
    // (all candidates run under ONE call number -- the caller's XMPI_ENTER: dsync_ll takes "the previous call was an agent's
    // collective and this is the next call" for "nothing was enqueued since", which the poison enqueued here would belie)
    std::lock_guard<std::mutex> g(c->coll_mu);
    c->dsync_split_bytes = cd.split ? 1 : 0;
    c->dsync_unroll = cd.unroll;
    const bool tr = trace_on() && per_rank >= ((size_t)64 << 20);
    const double tb = now_seconds();
    double t_arm = 0, t_run = 0, t_verdict = 0;
    // The check's rank-local kernels (poison, compare, refill) and a collective's WAITING kernels must not share the GPU: which ranks
    // poison or compare depends on the collective (bcast: everybody but the root; reduce: the root alone), so some ranks would be
    // spinning in the next collective's kernel while another still streams 256 MiB through a local one -- and with eight processes on
    // ONE GPU that mix stalled the tree kernels for 8 .. 60 s at a time (round-6 profiles/r06/tune_stall).  So every rank's local
    // kernels have ended, on every rank, before any rank launches a kernel that waits for a peer: stream sync + the job's barrier.
    auto settle = [&]() -> int {
      if (hipStreamSynchronize(c->local_stream) != hipSuccess) return hip_fail(hipGetLastError(), "hipStreamSynchronize", __FILE__, __LINE__);
      return job_barrier(c);
    };
    if (check) {
      rc = chk.arm(coll, per_rank);
      if (rc == XMPI_OK) rc = settle();
    }
    t_arm = now_seconds() - tb;
    double t0 = now_seconds();
    for (int i = -1; i < iters && rc == XMPI_OK; i++) {
      if (i == 0) t0 = now_seconds();
      rc = dsync_collective(c, coll, 0, coll == COLL_BCAST ? chk.recv : chk.send, chk.recv, per_rank / 4, XMPI_F32, XMPI_SUM, c->local_stream,
                            /*blocking=*/i == -1 || i == iters - 1, cd.algo);
      if (i == -1) t_run = now_seconds() - tb - t_arm;
      if (i == -1 && check && rc == XMPI_OK) {
        rc = chk.verdict(coll, per_rank, &bad[k]);
        t_verdict = now_seconds() - tb - t_arm - t_run;
        // ... and once more with the inputs changed in place -- whatever THIS rank's first verdict was: the ranks see different
        // verdicts (a wrong byte lands in one rank's buffer), and a run only some of them make is a hang
        if (rc == XMPI_OK && chk.twice && chk.second_pass(coll, per_rank)) {
          uint64_t bad2 = 0;
          rc = chk.change_inputs(coll, per_rank);
          if (rc == XMPI_OK) rc = chk.arm(coll, per_rank);
          if (rc == XMPI_OK) rc = settle();
          if (rc == XMPI_OK)
            rc = dsync_collective(c, coll, 0, coll == COLL_BCAST ? chk.recv : chk.send, chk.recv, per_rank / 4, XMPI_F32, XMPI_SUM, c->local_stream, true, cd.algo);
          if (rc == XMPI_OK) rc = chk.verdict(coll, per_rank, &bad2, /*second=*/true);
          // (every rank has left the run -- a blocking collective ends behind every peer's reads of this rank's buffers -- : refill)
          if (rc == XMPI_OK) rc = chk.restore_inputs(coll, per_rank);
          bad[k] = std::max(bad[k], bad2);
        }
        if (rc == XMPI_OK && iters > 0) rc = settle();  // ... before the timed runs
      }
    }
    if (iters > 0) {
      const double t_us = (now_seconds() - t0) / iters * 1e6;
      us[k] = keep_min && us[k] > 0 ? std::min(us[k], t_us) : t_us;
    }
    c->dsync_split_bytes = keep_split;
    c->dsync_unroll = keep_unroll;
    if (tr)
      fprintf(stderr, "[xmpi %d %.6f] tune:   %s %zu B by %s: %.0f us%s; arm %.1f ms, first run %.1f ms, verdict %.1f ms, all %.1f ms\n", c->rank, now_seconds(),
              coll_name(coll), per_rank, xmpi_comm::kCandName[k], iters > 0 ? us[k] : 0.0, check ? " (checked)" : "", t_arm * 1e3, t_run * 1e3, t_verdict * 1e3,
              (now_seconds() - tb) * 1e3);
    if (rc == XMPI_ERR_TIMEOUT && limit.keep == 0)
      set_last_error(std::string(coll_name(coll)) + " by " + xmpi_comm::kCandName[k] + " at " + std::to_string(per_rank) + " B per rank did not complete within " +
                     std::to_string(kTuneTimeoutS) + " s while the library was checking / timing it on this machine (" + xmpi_last_error() +
                     "): leave it out (xmpi_set_param \"tune_mask\") or give the job a no-progress limit (XMPI_TIMEOUT_S)");
  }
  return rc;
}

// What follows from a rejected schedule beyond "AUTO's table leaves it out": the untuned rules must not lead to it either.
static void apply_rejections(xmpi_comm* c) {
  uint32_t any = 0;
  for (int k = 0; k < 4; k++) any |= c->tune_rejected[k];
  if (any & (1u << xmpi_comm::CAND_LL)) {  // untuned AUTO sends short messages as LL lines
    c->ll_bytes = 0;
    c->agent_ll = 0;
    // (one mechanism -- 8-byte lines stored into the peers' flag allocations -- under all four collectives: wrong for one, trusted for none)
    for (int k = 0; k < 4; k++) c->tune_rejected[k] |= 1u << xmpi_comm::CAND_LL;
  }
  if (any & (1u << xmpi_comm::CAND_SPLIT)) c->dsync_split_bytes = 0;  // ... and large ones as meet / body / done
}

// The ladder's last rung: no device-synchronised schedule is right for some call on this machine -- the ranks meet on the host from
// now on (zcopy.cpp's rendezvous through the control block, the staged step tables), as after a flag page that could not be mapped.
// Collective (the caller's decision came out of a vote).
static void demote_to_host(xmpi_comm* c, const std::string& reason) {
  ll_agent_stop(c);
  (void)hipStreamSynchronize(c->local_stream);
  (void)hipGetLastError();
  c->dsync_ok = false;
  c->tuned = false;
  append(c->degraded_why, "the ranks meet on the host (no device-synchronised collectives): " + reason);
}

// what a check found: remembered, said (xmpi_degraded, xmpi_last_error, one line on stderr), and acted upon
static void note_rejections(xmpi_comm* c, const char* who, const std::string& why, bool none_right) {
  apply_rejections(c);
  if (why.empty() && !none_right) return;
  const std::string text = std::string(who) + ": " + why + (why.empty() ? "" : "; ") +
                           (none_right ? "no schedule left that is right for every call" : "left out of AUTO, refused by name (tune_rejected_<collective>)");
  append(c->rejected_why, text);
  append(c->degraded_why, text);
  if (none_right) demote_to_host(c, std::string(who) + " found no right schedule for some call");
  set_last_error(text);
  if (c->rank == 0) fprintf(stderr, "xmpi: degraded: %s\n", text.c_str());
}

// Send / Receive out of registered HBM straight into HBM -- the receiver's kernel LOADS the payload out of the sender's memory (the
// lingering receive agent up to 512 KiB, the pull kernel above: p2p.cpp p2p_recv) --: every rank sends `bytes` of its pattern to its
// right neighbour and counts what differs in what its left one sent (even ranks send first, odd ranks receive first: the blocking
// pair is a rendezvous, network.go:569).  Collective.
static int p2p_check_round(xmpi_comm* c, AnswerCheck& chk, size_t bytes, uint64_t* bad) {
  const int N = c->size, right = (c->rank + 1) % N, left = (c->rank + N - 1) % N;
  const int tag = 0x7fff5c5c;
  hipStream_t s = c->local_stream;
  *bad = 0;
  int rc = job_barrier(c);
  if (rc != XMPI_OK) return rc;
  XMPI_HIP(launch_fill(chk.expect, bytes / 4, XMPI_F32, kCheckPattern, kCheckSeed + (uint64_t)left, s));
  XMPI_HIP(launch_fill(chk.recv, bytes / 4, XMPI_F32, 2, 165, s));
  XMPI_HIP(hipStreamSynchronize(s));
  chk.have_coll = -1;
  size_t got = 0;
  {
    TuneTimeout limit(c);  // (as tune_measure: a message that never arrives is an error of the check, not a hang of Init)
    if (c->rank % 2 == 0) {
      rc = p2p_send(c, chk.send, bytes, XMPI_F32, right, tag);
      if (rc == XMPI_OK) rc = p2p_recv(c, chk.recv, bytes, XMPI_F32, left, tag, &got);
    } else {
      rc = p2p_recv(c, chk.recv, bytes, XMPI_F32, left, tag, &got);
      if (rc == XMPI_OK) rc = p2p_send(c, chk.send, bytes, XMPI_F32, right, tag);
    }
  }
  if (rc != XMPI_OK) return rc;
  if (got != bytes) {
    *bad = bytes;
    return XMPI_OK;
  }
  XMPI_HIP(launch_signal(c->dev_words, 0, s));
  XMPI_HIP(launch_count_mismatch(chk.recv, chk.expect, bytes, c->dev_words, s));
  XMPI_HIP(chk.count_to_host(bad));
  return XMPI_OK;
}

// The ladder's first rung: meet / body / done gave wrong answers with the data kernel that relies on the meet and done kernels'
// acquire / release once per XCD -- its system-scope form relies on nothing (what the XCD probe would have chosen).  body_sys is
// set, the split candidate runs (checked, then `iters` times against the clock into us[], if there is one) and is voted on again;
// what every rank then holds of it replaces worst[] (if there is one) and worst_bad[]; still wrong: body_sys is put back.  Collective.
static int split_with_body_sys(xmpi_comm* c, AnswerCheck& chk, const std::vector<TuneCand>& cands, int coll, size_t per_rank, int iters, double* us,
                               uint64_t* bad, double* worst, uint64_t* worst_bad, std::string& why) {
  const int S = xmpi_comm::CAND_SPLIT;
  const uint64_t first = worst_bad[S];
  c->body_sys = 1;
  if (us) us[S] = 0;
  bad[S] = 0;
  int rc = tune_measure(c, chk, cands, coll, per_rank, {S}, iters, true, false, us, bad);
  std::vector<double> w2(cands.size(), 0.0);
  std::vector<uint64_t> b2(cands.size(), 0);
  if (rc == XMPI_OK) rc = vote_max(c, us, bad, (int)cands.size(), worst ? w2.data() : nullptr, b2.data());
  if (rc != XMPI_OK) return rc;
  char t[200];
  snprintf(t, sizeof t, "%s: split gave wrong answers at %zu B per rank (%llu bytes differ on the worst rank); its system-scope data kernel %s",
           coll_name(coll), per_rank, (unsigned long long)first, b2[S] ? "does too" : "is right and takes over (body_sys)");
  append(why, t);
  if (worst) worst[S] = w2[S];
  worst_bad[S] = b2[S];
  if (b2[S]) c->body_sys = 0;
  return XMPI_OK;
}

// xmpi_init's self-check (XMPI_SELFCHECK; default: on when the ranks sit on different GPUs): what UNTUNED AUTO can reach -- LL lines
// up to ll_bytes, the one-kernel fold, meet / body / done -- runs once, multi-tile, on patterned inputs before the first caller's
// data does; the other three collectives' folds ride along.  A job that tunes (xmpi_tune, XMPI_AUTOTUNE_BYTES) checks every
// candidate at every size anyway.  Collective.
int init_selfcheck(xmpi_comm* c) {
  const double t_begin = now_seconds();
  t_api_call = c->api_calls.fetch_add(1, std::memory_order_relaxed) + 1;  // (as a public call: XMPI_ENTER)
  // the diagnostic counters count the CALLER's traffic (tests and benchmarks read them as such): what the check itself moves is taken out again
  // (the receive agent's launches are NUMBERED by a counter of their own -- p2p_agent_launch_no, agent.cpp agent_submit -- which goes on counting)
  typedef uint64_t xmpi_comm::*Counter;
  static const Counter kCounters[13] = {&xmpi_comm::p2p_direct_count, &xmpi_comm::p2p_staged_count, &xmpi_comm::p2p_lane_count, &xmpi_comm::p2p_agent_served,
                                        &xmpi_comm::p2p_agent_launches, &xmpi_comm::dsync_launches, &xmpi_comm::dsync_ll_launches, &xmpi_comm::dsync_ll_agent,
                                        &xmpi_comm::ll_agent_launches, &xmpi_comm::dsync_split_launches, &xmpi_comm::dsync_sched_launches,
                                        &xmpi_comm::dsync_bounced, &xmpi_comm::host_bounce_calls};
  uint64_t before[13];
  for (int k = 0; k < 13; k++) before[k] = c->*kCounters[k];
  // several 4 KiB tiles per rank's chunk at 8 ranks (fold: 4; split: 8 one-tile blocks, one per XCD); bcast just above
  // zc_bcast_push_bytes, where every rank forwards its chunk
  const size_t kFold = (size_t)128 << 10, kSplit = (size_t)256 << 10;
  const size_t kBcast = (size_t)std::max<long>(0, c->zc_bcast_push_bytes) + 16384 <= kSplit * 2 ? (size_t)std::max<long>(0, c->zc_bcast_push_bytes) + 16384 : kSplit;
  const size_t kP2PShort = (size_t)64 << 10, kP2PLong = (size_t)768 << 10;  // the receive agent's side of its 512 KiB limit, and the pull kernel's
  AnswerCheck chk;
  int rc;
  {
    std::lock_guard<std::mutex> g(c->coll_mu);
    rc = chk.open(c, std::max(std::max(kSplit, kBcast), kP2PLong));
  }
  if (rc != XMPI_OK) return rc;
  XMPI_TRACE_STEP(c->rank, "self-check: buffers ready");
  // (what the job's first xmpi_malloc and first kernel pay anyway -- the first arena allocated, exported, mapped by every peer;
  // the code object loaded -- reported apart from the checks themselves)
  c->selfcheck_setup_ms = (now_seconds() - t_begin) * 1e3;
  const std::vector<TuneCand> cands = tune_candidates(c);
  c->tune_running = true;
  std::string why;
  bool fold_wrong = false;
  auto run = [&](int coll, size_t per_rank, std::vector<int> ks, uint64_t* worst_bad) -> int {
    std::vector<uint64_t> bad(cands.size(), 0);
    {
      std::lock_guard<std::mutex> g(c->coll_mu);
      rc = chk.expect_for(coll, per_rank);
    }
    if (rc == XMPI_OK) rc = tune_measure(c, chk, cands, coll, per_rank, ks, 0, true, false, nullptr, bad.data());
    if (rc == XMPI_OK) rc = vote_max(c, nullptr, bad.data(), (int)cands.size(), nullptr, worst_bad);
    return rc;
  };
  auto reject = [&](int coll, int k, size_t per_rank, uint64_t nbad) {
    c->tune_rejected[coll] |= 1u << k;
    append(why, wrong_answers(coll, k, "", per_rank, nbad));
  };
  std::vector<uint64_t> wb(cands.size(), 0);
  do {
    // allreduce: LL lines, the one-kernel fold, meet / body / done
    const size_t ll = (size_t)std::min<long>(c->ll_bytes, 4096) / 16 * 16;
    if (ll >= 16) {
      if ((rc = run(COLL_ALLREDUCE, ll, {xmpi_comm::CAND_LL}, wb.data())) != XMPI_OK) break;
      if (wb[xmpi_comm::CAND_LL]) reject(COLL_ALLREDUCE, xmpi_comm::CAND_LL, ll, wb[xmpi_comm::CAND_LL]);
    }
    XMPI_TRACE_STEP(c->rank, "self-check: LL lines done");
    if ((rc = run(COLL_ALLREDUCE, kFold, {xmpi_comm::CAND_FOLD}, wb.data())) != XMPI_OK) break;
    XMPI_TRACE_STEP(c->rank, "self-check: fold done");
    if (wb[xmpi_comm::CAND_FOLD]) {
      reject(COLL_ALLREDUCE, xmpi_comm::CAND_FOLD, kFold, wb[xmpi_comm::CAND_FOLD]);
      fold_wrong = true;
    }
    if (c->dsync_split_bytes > 0) {
      if ((rc = run(COLL_ALLREDUCE, kSplit, {xmpi_comm::CAND_SPLIT}, wb.data())) != XMPI_OK) break;
      if (wb[xmpi_comm::CAND_SPLIT] && !c->body_sys) {
        std::vector<uint64_t> bad(cands.size(), 0);
        if ((rc = split_with_body_sys(c, chk, cands, COLL_ALLREDUCE, kSplit, 0, nullptr, bad.data(), nullptr, wb.data(), why)) != XMPI_OK) break;
      }
      if (wb[xmpi_comm::CAND_SPLIT]) reject(COLL_ALLREDUCE, xmpi_comm::CAND_SPLIT, kSplit, wb[xmpi_comm::CAND_SPLIT]);
    }
    XMPI_TRACE_STEP(c->rank, "self-check: split done");
    // the other collectives' folds (other segment tables of the same kernel; bcast above zc_bcast_push_bytes: scatter + allgather)
    for (int coll : {(int)COLL_REDUCE, (int)COLL_ALLGATHER, (int)COLL_BCAST}) {
      const size_t per_rank = coll == COLL_ALLGATHER ? kFold / (size_t)c->size / 16 * 16 : coll == COLL_BCAST ? kBcast : kFold;
      if ((rc = run(coll, per_rank, {xmpi_comm::CAND_FOLD}, wb.data())) != XMPI_OK) break;
      if (wb[xmpi_comm::CAND_FOLD]) {
        reject(coll, xmpi_comm::CAND_FOLD, per_rank, wb[xmpi_comm::CAND_FOLD]);
        fold_wrong = true;
      }
    }
    if (rc != XMPI_OK) break;
    // Send / Receive: the receiver's direct pull out of the sender's registered memory, short (agent) and long (pull kernel).  Wrong:
    // the messages travel through the mail slots of the windows instead (p2p_direct_bytes < 0: pushed by the sender's copy engine,
    // drained locally -- two copies, no load over a link), checked in turn; wrong again, or no windows: xmpi_init fails on every rank.
    for (int attempt = 0; attempt < 2 && rc == XMPI_OK; attempt++) {
      uint64_t mine[2] = {0, 0}, worst[2] = {0, 0};
      if ((rc = p2p_check_round(c, chk, kP2PShort, &mine[0])) != XMPI_OK) break;
      if ((rc = p2p_check_round(c, chk, kP2PLong, &mine[1])) != XMPI_OK) break;
      if ((rc = vote_max(c, nullptr, mine, 2, nullptr, worst)) != XMPI_OK) break;
      if (!worst[0] && !worst[1]) break;
      char t[240];
      snprintf(t, sizeof t, "Send / Receive: %s gives wrong answers on this machine (%llu of %zu / %llu of %zu bytes differ on the worst rank)",
               attempt == 0 ? "the receiver's direct pull out of the sender's registered memory" : "the mail slots too", (unsigned long long)worst[0], kP2PShort,
               (unsigned long long)worst[1], kP2PLong);
      append(why, t);
      if (attempt == 0 && c->windows_ok && c->p2p_direct_bytes >= 0) {
        c->p2p_direct_bytes = -1;
        c->p2p_rejected |= 1u;
        why += ": messages travel through the mail slots";
        continue;
      }
      c->p2p_rejected |= 2u;
      set_last_error("xmpi_init self-check: " + why + ": no way left to move a message between GPUs that gives right answers");
      rc = XMPI_ERR_HIP;
    }
  } while (false);
  c->tune_running = false;
  {
    std::lock_guard<std::mutex> g(c->coll_mu);
    chk.close();
  }
  if (rc != XMPI_OK) {
    if (c->rank == 0 && (c->p2p_rejected & 2u)) fprintf(stderr, "xmpi: %s\n", xmpi_last_error());
    if (!(c->p2p_rejected & 2u)) c->ctl->set_abort(rc);  // (a verdict every rank reached together needs no abort; a failure of this rank alone does)
    return rc;
  }
  // an untuned job has no table to route round a wrong fold: the one-kernel fold is what every collective's AUTO comes down to
  note_rejections(c, "xmpi_init self-check", why, fold_wrong);
  for (int k = 0; k < 13; k++) c->*kCounters[k] = before[k];
  c->selfcheck_ms = (now_seconds() - t_begin) * 1e3;
  return job_barrier(c);
}
}  // namespace xmpi

using namespace xmpi;

extern "C" {

// ---- the library's own schedule table ---------------------------------------------------------------------------------

// Which of n candidates (mean times in microseconds; <= 0 = did not run) AUTO should take: the fastest -- but the default
// (index 0) stays unless another one beats it by more than `margin` (a fraction: noise must not flip the schedule).
int xmpi_tune_decide(const double* us, int n, double margin) {
  if (!us || n < 1) return -1;
  int best = -1;
  for (int i = 0; i < n; i++)
    if (us[i] > 0 && (best < 0 || us[i] < us[best])) best = i;
  if (best < 0) return -1;
  if (best != 0 && us[0] > 0 && us[best] >= us[0] * (1.0 - (margin > 0 ? margin : 0.0))) return 0;
  return best;
}

// Times the schedules this job's layout offers for allreduce-sum f32, allgather, bcast and reduce on the real buffers, size class by size
// class -- after CHECKING each one's answer at that size (above) --, lets every rank see the same (max over ranks) figures and fills the
// table AUTO consults (dsync_plan.cpp dsync_route).  A candidate that was wrong on ANY rank at ANY size leaves the collective's table on
// EVERY rank (xmpi_get_param "tune_rejected_<collective>", xmpi_degraded(), xmpi_last_error()); a wrong DEFAULT walks the ladder the
// mapping vote walks: split -> its system-scope data kernel -> the one-kernel fold -> (no right schedule left for some size) the ranks
// meet on the host.  Collective: every rank calls it with the same max_bytes.  With ranks that meet on the host there is nothing to choose.
int xmpi_tune(xmpi_comm* c, size_t max_bytes) {
  XMPI_ENTER(c);
  drain_worker(c);
  if (!dsync_usable(c) || c->size < 2) return XMPI_OK;
  const double t_begin = now_seconds();
  max_bytes = std::min<size_t>(std::max<size_t>(max_bytes, 1024), (size_t)1 << 30);
  AnswerCheck chk;
  int rc;
  {
    std::lock_guard<std::mutex> g(c->coll_mu);
    rc = chk.open(c, max_bytes);
  }
  if (rc != XMPI_OK) return rc;
  const std::vector<TuneCand> cands = tune_candidates(c);
  const long keep_split = c->dsync_split_bytes;
  const bool keep_tuned = c->tuned;
  c->tuned = false;
  c->tune_running = true;
  memset(c->tune_algo, -1, sizeof c->tune_algo);
  memset(c->tune_split, -1, sizeof c->tune_split);
  memset(c->tune_unroll, 0, sizeof c->tune_unroll);
  memset(c->tune_rejected, 0, sizeof c->tune_rejected);
  std::string why;
  bool none_right = false;
  struct Row {
    size_t per_rank;
    std::vector<double> worst;
  };
  std::vector<Row> all_rows[4];
  uint32_t ll_out = 0;  // LL lines are ONE mechanism under all four collectives: wrong for one, trusted for none (apply_rejections)
  for (int coll : {(int)COLL_ALLREDUCE, (int)COLL_REDUCE, (int)COLL_ALLGATHER, (int)COLL_BCAST}) {  // (the two that share the expected sum side by side)
    std::vector<Row>& rows = all_rows[coll];
    uint32_t rejected = ll_out;
    for (size_t bytes = 1024; bytes <= max_bytes && rc == XMPI_OK; bytes *= 4) {
      const size_t per_rank = coll == COLL_ALLGATHER ? bytes / (size_t)c->size / 16 * 16 : bytes;
      if (per_rank < 16) continue;
      // (XMPI_TUNE_ITERS: a cap on the timed runs per candidate -- the rehearsals on virtual devices, where a "kernel" is a host thread and
      // a time means nothing, keep every candidate's CHECKED run and pay for two timed ones)
      static const long iters_cap = env_long("XMPI_TUNE_ITERS", 0);
      const int by_size = bytes <= ((size_t)1 << 20) ? 20 : (bytes <= ((size_t)32 << 20) ? 6 : 3);
      const int iters = iters_cap > 0 ? (int)std::min<long>(by_size, iters_cap) : by_size;
      std::vector<double> us(cands.size(), 0.0), worst(cands.size(), 0.0);
      std::vector<uint64_t> bad(cands.size(), 0), worst_bad(cands.size(), 0);
      std::vector<int> ks;
      for (size_t k = 0; k < cands.size(); k++) {
        if (!tune_offered(c, coll, cands[k])) continue;
        if (cands[k].algo == XMPI_ALGO_LL && per_rank > kLLMaxPayload) continue;
        if (k > 0 && !((c->tune_mask >> k) & 1)) continue;  // a schedule the caller has ruled out on this machine (never the default)
        if ((rejected >> k) & 1u) continue;                 // ... or a smaller size has (the vote: the same on every rank)
        ks.push_back((int)k);
      }
      {
        std::lock_guard<std::mutex> g(c->coll_mu);
        rc = chk.expect_for(coll, per_rank);
      }
      // few iterations fit a large message into a tuning budget, and a few iterations are noisy (eight processes on one GPU:
      // +-6 % between two runs of one schedule): large sizes are measured twice, the candidates interleaved, and the better
      // figure of each counts
      const int rounds = bytes > ((size_t)1 << 20) ? 2 : 1;
      // (the check's second pass -- inputs changed in place -- at every other size up to 1 MiB: 4 KiB, 64 KiB, 1 MiB; halves what it costs)
      chk.twice = bytes == ((size_t)4 << 10) || bytes == ((size_t)64 << 10) || bytes == ((size_t)1 << 20);
      for (int round = 0; round < rounds && rc == XMPI_OK; round++)
        rc = tune_measure(c, chk, cands, coll, per_rank, ks, iters, /*check=*/round == 0, /*keep_min=*/round > 0, us.data(), bad.data());
      if (rc != XMPI_OK) break;
      // every rank must read the same figures: the slowest rank's times, the worst rank's answers
      rc = vote_max(c, us.data(), bad.data(), (int)cands.size(), worst.data(), worst_bad.data());
      if (rc != XMPI_OK) break;
      if (worst_bad[xmpi_comm::CAND_SPLIT] && !c->body_sys) {
        rc = split_with_body_sys(c, chk, cands, coll, per_rank, iters, us.data(), bad.data(), worst.data(), worst_bad.data(), why);
        if (rc != XMPI_OK) break;
      }
      for (size_t k = 0; k < cands.size(); k++)
        if (worst_bad[k] && !((rejected >> k) & 1u)) {
          rejected |= 1u << k;
          append(why, wrong_answers(coll, (int)k, "first at ", per_rank, worst_bad[k]));
        }
      rows.push_back({per_rank, worst});
      if (trace_on()) fprintf(stderr, "[xmpi %d %.6f] tune: %s %zu B per rank done\n", c->rank, now_seconds(), coll_name(coll), per_rank);
    }
    if (rc != XMPI_OK) break;
    c->tune_rejected[coll] = rejected;
    ll_out |= rejected & (1u << xmpi_comm::CAND_LL);
  }
  // the tables, once the rejected sets are known: what was wrong at one size is not trusted at another
  for (int coll = 0; coll < 4 && rc == XMPI_OK; coll++) {
    std::vector<Row>& rows = all_rows[coll];
    const uint32_t rejected = c->tune_rejected[coll] | ll_out;
    for (size_t ri = 0; ri < rows.size(); ri++) {
      const size_t per_rank = rows[ri].per_rank;
      std::vector<double>& worst = rows[ri].worst;
      bool ran = false;
      for (size_t k = 0; k < cands.size(); k++) {
        ran = ran || worst[k] > 0;
        if ((rejected >> k) & 1u) worst[k] = 0;
      }
      // "the default stays on a tie" -- and the untuned library already runs meet / body / done from dsync_split_bytes on: there
      // candidate 2 is the default, so it is decided with the two swapped
      // (what dsync_split_bytes is compared with: the bytes one rank's kernel moves -- dsync.cpp launch_fold)
      const size_t moved = coll == COLL_ALLREDUCE ? 2 * per_rank : coll == COLL_REDUCE ? per_rank / (size_t)c->size * (size_t)(c->size + 1)
                           : coll == COLL_ALLGATHER ? per_rank * (size_t)(c->size + 1) : 0;
      const bool split_is_default = keep_split > 0 && moved >= (size_t)keep_split && worst[2] > 0;
      if (split_is_default) std::swap(worst[0], worst[2]);
      int best = xmpi_tune_decide(worst.data(), (int)worst.size(), 0.03);
      if (split_is_default && (best == 0 || best == 2)) best = 2 - best;
      if (best < 0) {
        if (ran) none_right = true;  // every schedule this collective has at this size is wrong here
        continue;
      }
      int k = 0;
      while (k + 1 < xmpi_comm::kTuneClasses && (per_rank >> (k + 9)) != 0) k++;
      const TuneCand& won = cands[(size_t)best];
      // this class and the one to the next measured size; beyond the largest measured size: what won there
      for (int kk = k; kk < xmpi_comm::kTuneClasses; kk++) set_row(c, coll, kk, won);
      if (ri == 0)  // below the smallest measured size: what won there
        for (int kk = 0; kk < k; kk++) set_row(c, coll, kk, won);
    }
  }
  c->tune_running = false;
  {
    std::lock_guard<std::mutex> g(c->coll_mu);
    chk.close();
  }
  c->tune_check_ms = chk.spent_s * 1e3;
  if (rc != XMPI_OK) {
    c->tuned = keep_tuned;
    c->ctl->set_abort(rc);  // (the other ranks are in, or on their way to, a barrier of this very call: they must not wait for this one)
    return rc;
  }
  c->tuned = true;
  note_rejections(c, "xmpi_tune", why, none_right);
  rc = xmpi_barrier(c);
  c->tune_ms = (now_seconds() - t_begin) * 1e3;
  return rc;
}

}  // extern "C"
