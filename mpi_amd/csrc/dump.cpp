// dump.cpp -- the schedules as text and figures (host logic only): what tests/sched_sim.py and the plan tests read.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "comm.h"
#include "kernels.h"
#include "sched_steps.h"

using namespace xmpi;

// as much of `t` as fits into out[cap], terminated; returns the needed length
static int text_out(const std::string& t, char* out, size_t cap) {
  if (out && cap) {
    const size_t n = std::min(cap - 1, t.size());
    memcpy(out, t.data(), n);
    out[n] = 0;
  }
  return (int)std::min<size_t>(t.size() + 1, 0x7fffffff);
}

extern "C" {

int xmpi_zc_chunk(size_t count, size_t elem_size, int size, int j, size_t* elem_off, size_t* elem_cnt) {
  if (!elem_off || !elem_cnt || size < 1 || j < 0 || j >= size || elem_size < 1) return XMPI_ERR_ARG;
  zc_chunk(count, elem_size, size, j, elem_off, elem_cnt);
  return XMPI_OK;
}

// The step program a stepped kernel (sched.hip) runs on `rank` for ring channel `channel`, as text -- produced by the very
// function the kernel calls (sched_steps.h).  One line per step:
//   g wait=<rank>:<value> sig=<rank>,<rank>:<value> nmv=<moves> then per move
//   | ns=<1|2|3> D=<ref> D2=<ref> A=<ref> B=<ref> C=<ref> lo=<byte> hi=<byte>        ref = <rank>.<s|r|l><+offset> or -
// (s = send buffer, r = receive buffer, l = landing block).  form: 0 = pull, 1 = push; in_place: every rank's send buffer is its
// receive buffer (what decides whether a push-form ring lands in the receive buffers or in landing blocks).
// (host logic only; tests/sched_sim.py executes all ranks' programs on the CPU).  Returns the needed length.
int xmpi_sched_dump(int sched, int form, int in_place, int size, int rank, int root, int pieces, size_t count, size_t elem_size, int nchan,
                    int channel, char* out, size_t cap) {
  if (size < 1 || size > kDsyncRanks || rank < 0 || rank >= size || root < 0 || root >= size || elem_size < 1 || nchan < 1 ||
      nchan > kMaxSchedChannels || channel < 0 || channel >= nchan || sched < SCHED_RING_ALLREDUCE || sched > SCHED_TREE_REDUCE ||
      form < 0 || form > 1 || (sched == SCHED_TREE_REDUCE && pieces > 127))  // (a step number must fit the low byte of a flag word)
    return XMPI_ERR_ARG;
  DsyncSchedArgs a;
  memset(&a, 0, sizeof a);
  a.d.me = rank;
  a.d.n = size;
  a.sched = sched;
  a.push = (uint32_t)form;
  a.nchan = nchan;
  a.root = root;
  a.pieces = std::max(1, pieces);
  a.count = count;
  a.elem_size = (uint32_t)elem_size;
  for (int ch = 0; ch < nchan; ch++) {
    std::vector<int> ord;
    ring_order(size, ch, &ord);
    for (int i = 0; i < size; i++) a.order[ch][i] = (uint8_t)ord[(size_t)i];
  }
  // recognisable addresses: rank r's send / receive buffer / landing block = ((r+1) << 44) | (kind << 42) | 2^41 (+ a signed offset)
  uint64_t send[kDsyncRanks], recv[kDsyncRanks], land[kDsyncRanks];
  auto fake = [](int r, int kind) { return ((uint64_t)(r + 1) << 44) | ((uint64_t)kind << 42) | (1ull << 41); };
  for (int r = 0; r < size; r++) {
    // in place: the send buffer IS the receive buffer (tree reduce: at the root only -- nobody else has one; allgather: the
    // rank's block of it)
    recv[r] = fake(r, 1);
    send[r] = !in_place || sched == SCHED_TREE_BCAST || (sched == SCHED_TREE_REDUCE && r != root) ? fake(r, 0)
              : sched == SCHED_RING_ALLGATHER           ? recv[r] + (uint64_t)r * count * elem_size
                                                        : recv[r];
    DsyncSchedArgs ar = a;
    ar.d.me = r;
    land[r] = sched_land_bytes(ar, in_place != 0) ? fake(r, 2) : 0;  // (as dsync_call.cpp DsyncCall::own_block lends them)
  }
  auto show = [&](uint64_t base, char* buf, size_t n) {
    if (!base) {
      snprintf(buf, n, "-");
      return;
    }
    const int r = (int)(base >> 44) - 1, kind = (int)((base >> 42) & 3);
    const long long off = (long long)(base - fake(r, kind));
    snprintf(buf, n, "%d.%c%+lld", r, "srl?"[kind], off);
  };
  std::string t;
  const int ns = sched_nsteps(a);
  for (int g = 1; g <= ns; g++) {
    SchedStep st;
    sched_step(a, send, recv, land, g, channel, &st);
    char line[160];
    snprintf(line, sizeof line, "%d wait=%d:%u sig=%d,%d:%u nmv=%d", g, st.wait_rank, st.wait_val, st.sig[0], st.sig[1], st.sig_val, st.nmv);
    t += line;
    for (int k = 0; k < st.nmv; k++) {
      const SchedMove& m = st.mv[k];
      char d[48], d2[48], x[48], y[48], z[48], mv[400];
      show(m.D, d, sizeof d);
      show(m.D2, d2, sizeof d2);
      show(m.A, x, sizeof x);
      show(m.ns >= 2 ? m.B : 0, y, sizeof y);
      show(m.ns >= 3 ? m.C : 0, z, sizeof z);
      snprintf(mv, sizeof mv, " | ns=%d D=%s D2=%s A=%s B=%s C=%s lo=%llu hi=%llu", m.ns, d, d2, x, y, z, (unsigned long long)m.lo,
               (unsigned long long)m.hi);
      t += mv;
    }
    t += "\n";
  }
  return text_out(t, out, cap);
}

size_t xmpi_sched_land_bytes(int sched, int in_place, int size, int rank, int root, size_t count, size_t elem_size) {
  if (size < 1 || size > kDsyncRanks || rank < 0 || rank >= size || root < 0 || root >= size) return 0;
  DsyncSchedArgs a;
  memset(&a, 0, sizeof a);
  a.d.me = rank;
  a.d.n = size;
  a.sched = sched;
  a.push = 1;
  a.root = root;
  a.count = count;
  a.elem_size = (uint32_t)elem_size;
  return (size_t)sched_land_bytes(a, in_place != 0);
}

int xmpi_plan_dump(int coll, int algo, int size, int rank, int root, size_t count, size_t elem_size, int channels,
                   size_t piece_elems, int fifo_depth, size_t oneshot_bytes, char* out, size_t cap) {
  PlanParams pp;
  pp.coll = coll;
  pp.algo = (algo == XMPI_ALGO_ZCOPY || algo == XMPI_ALGO_ZPUSH) ? (int)XMPI_ALGO_AUTO : algo;  // the staged fallback
  pp.size = size;
  pp.rank = rank;
  pp.root = root;
  pp.count = count;
  pp.elem_size = elem_size;
  pp.channels = channels;
  pp.lanes = 2;
  pp.piece_bytes = piece_elems * elem_size;
  pp.fuse = 1;
  pp.fifo_depth = fifo_depth > 0 ? fifo_depth : 8;  // (0: the library's defaults)
  pp.oneshot_bytes = oneshot_bytes != (size_t)-1 ? oneshot_bytes : (size_t)1 << 20;
  Plan plan;
  int rc = build_plan(pp, &plan);
  if (rc != XMPI_OK) return rc;
  const std::string t = plan_to_text(plan);
  return text_out(t, out, cap);
}

}  // extern "C"
