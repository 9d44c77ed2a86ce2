// tests/devsim/driver_vcoll.cpp -- xmpi_alltoallv with the ranks as THREADS of this process, every rank on a virtual HIP device of
// its own (tests/devsim), driven through the C ABI of include/xmpi.h: the kernel that reads the counts and exchanges them between
// the ranks (kernels.hip dsync_alltoallv_kernel) and the v-box protocol (kernels.h VBox: single-buffered, rewritten at the next
// call) under -fsanitize=thread and, in a second build, -fsanitize=undefined (tests/test_vcoll_devsim.py builds both).
//
// The exchange is the one the reference's own program performs (helloworld.go:53-81; Receive re-sizes, network.go:594-601).
//
// usage: driver_vcoll <ranks> <rounds>      --shared <ranks> <rounds>: every rank on device 0 (the ranks meet on the host)
// exit 0 = every result was right; the sanitizers report on stderr (TSAN_OPTIONS=exitcode=66)
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xmpi.h"

namespace {

std::atomic<int> g_bad{0};
bool g_shared = false;

#define CHECK(call)                                                                                              \
  do {                                                                                                           \
    const int _rc = (call);                                                                                      \
    if (_rc != XMPI_OK) {                                                                                        \
      fprintf(stderr, "rank %d: %s:%d: %s -> %d (%s)\n", rank, __FILE__, __LINE__, #call, _rc, xmpi_last_error()); \
      g_bad.fetch_add(1);                                                                                        \
      return;                                                                                                    \
    }                                                                                                            \
  } while (0)

const uint64_t kCounts[] = {0, 1, 3, 17, 1000, 4099, 20011};
inline uint64_t count_of(int from, int to, int salt, int size) {
  if (from == salt % size || to == (salt + 1) % size) return 0;
  return kCounts[(from * 5 + to * 3 + salt) % 7];  // (5 and 3 are coprime to 7: the sender and the receiver both count)
}
inline uint8_t byte_of(int from, uint64_t at) { return (uint8_t)((at * 31 + (uint64_t)from * 17 + (at >> 9)) & 0xff); }

// the arrays of one rank, in elements: every block at a multiple of 16 elements plus a residue (0 / 0: packets; 3 / 3 with one-byte
// elements: head, packets, tail; 1 / 6: one element per lane)
struct Plan {
  std::vector<uint64_t> sc, sd, caps, rd;
  uint64_t se = 0, re = 0;
};
Plan plan_of(int rank, int size, int salt, int rs, int rr, uint64_t slack) {
  Plan p;
  uint64_t at = 0;
  for (int j = 0; j < size; j++) {
    p.sc.push_back(count_of(rank, j, salt, size));
    p.sd.push_back(at + (uint64_t)rs);
    at += (p.sc.back() + (uint64_t)rs + 15) / 16 * 16;
  }
  p.se = at;
  at = 0;
  for (int r = 0; r < size; r++) {
    p.caps.push_back(count_of(r, rank, salt, size) + slack);
    p.rd.push_back(at + (uint64_t)rr);
    at += (p.caps.back() + (uint64_t)rr + 15) / 16 * 16;
  }
  p.re = at;
  return p;
}

struct Rank {
  int rank, size;
  xmpi_comm* c = nullptr;
  void *send = nullptr, *recv = nullptr;
  uint64_t* dev = nullptr;  // the five arrays in device memory (stream form)
  std::vector<uint8_t> host;

  void fill(size_t send_bytes, size_t recv_bytes) {
    host.resize(send_bytes);
    for (size_t i = 0; i < send_bytes; i++) host[i] = byte_of(rank, i);
    (void)xmpi_memcpy(c, send, host.data(), send_bytes);
    (void)xmpi_memset(c, recv, 0xA5, recv_bytes + 64);
  }
  // the whole receive buffer, the gaps and the 64 bytes behind it included
  void expect(int salt, int rs, int rr, uint64_t slack, size_t es, const uint64_t* got, int cut_from, const char* what) {
    const Plan mine = plan_of(rank, size, salt, rs, rr, slack);
    std::vector<uint8_t> want(mine.re * es + 64, 0xA5), out(mine.re * es + 64);
    for (int r = 0; r < size; r++) {
      const Plan theirs = plan_of(r, size, salt, rs, rr, slack);
      if (got[r] != theirs.sc[(size_t)rank]) {
        fprintf(stderr, "rank %d: %s: recvcounts[%d] = %llu, expected %llu\n", rank, what, r, (unsigned long long)got[r], (unsigned long long)theirs.sc[(size_t)rank]);
        g_bad.fetch_add(1);
        return;
      }
      if (r == cut_from) continue;
      for (uint64_t i = 0; i < theirs.sc[(size_t)rank] * es; i++) want[mine.rd[(size_t)r] * es + i] = byte_of(r, theirs.sd[(size_t)rank] * es + i);
    }
    (void)xmpi_memcpy(c, out.data(), recv, out.size());
    for (size_t i = 0; i < out.size(); i++)
      if (out[i] != want[i]) {
        fprintf(stderr, "rank %d: %s salt %d: byte %zu of the receive buffer is %u, expected %u\n", rank, what, salt, i, out[i], want[i]);
        g_bad.fetch_add(1);
        return;
      }
  }
};

void rank_main(const std::string& key, int rank, int size, int rounds) {
  Rank R;
  R.rank = rank;
  R.size = size;
  CHECK(xmpi_init(rank, size, g_shared ? 0 : rank, key.c_str(), &R.c));
  xmpi_comm* c = R.c;
  if (!g_shared && xmpi_get_param(c, "dsync") != 1) {
    fprintf(stderr, "rank %d: the ranks do not meet on the device: nothing of interest would run\n", rank);
    g_bad.fetch_add(1);
    return;
  }
  const size_t cap_bytes = (size_t)size * (20011 + 64) * 8 + 64;
  R.send = xmpi_malloc(c, cap_bytes);
  R.recv = xmpi_malloc(c, cap_bytes);
  R.dev = (uint64_t*)xmpi_malloc(c, 5 * 16 * sizeof(uint64_t));
  void* small_s = xmpi_malloc(c, (size_t)size * 64 * 4);
  void* small_r = xmpi_malloc(c, (size_t)size * 64 * 4);
  if (!R.send || !R.recv || !R.dev || !small_s || !small_r) {
    g_bad.fetch_add(1);
    return;
  }
  (void)xmpi_memset(c, small_s, 1, (size_t)size * 64 * 4);
  std::vector<uint64_t> got((size_t)size);
  void* s = g_shared ? nullptr : xmpi_stream_create(c);
  int salt = 0;
  const long v0 = xmpi_get_param(c, "dsync_v_launches");
  for (int round = 0; round < rounds; round++) {
    struct Shape { xmpi_dtype dt; size_t es; int rs, rr; };
    for (const Shape sh : {Shape{XMPI_U8, 1, 0, 0}, Shape{XMPI_U8, 1, 3, 3}, Shape{XMPI_U8, 1, 1, 6}, Shape{XMPI_F16, 2, 0, 0}, Shape{XMPI_I64, 8, 0, 0}, Shape{XMPI_I64, 8, 1, 1}}) {
      for (int algo : {(int)XMPI_ALGO_AUTO, (int)XMPI_ALGO_DIRECT}) {
        const Plan p = plan_of(rank, size, ++salt, sh.rs, sh.rr, 5);
        R.fill(p.se * sh.es, p.re * sh.es);
        CHECK(xmpi_alltoallv(c, R.send, p.se, p.sc.data(), p.sd.data(), R.recv, p.re, p.caps.data(), p.rd.data(), got.data(), sh.dt, algo));
        R.expect(salt, sh.rs, sh.rr, 5, sh.es, got.data(), -1, "alltoallv");
      }
    }
    // back to back, other collectives in between: the v-boxes are rewritten at the next call, the LL slots keep their parity
    for (int k = 0; k < 6; k++) {
      const Plan p = plan_of(rank, size, ++salt, 0, 0, 0);
      R.fill(p.se * 2, p.re * 2);
      CHECK(xmpi_alltoallv(c, R.send, p.se, p.sc.data(), p.sd.data(), R.recv, p.re, p.caps.data(), p.rd.data(), got.data(), XMPI_F16, XMPI_ALGO_AUTO));
      CHECK(xmpi_alltoall(c, small_s, small_r, 64, XMPI_I32, XMPI_ALGO_LL));
      CHECK(xmpi_allreduce(c, small_s, small_r, 64, XMPI_I32, XMPI_SUM, XMPI_ALGO_AUTO));
      R.expect(salt, 0, 0, 0, 2, got.data(), -1, "alltoallv, back to back");
    }
    // a pair over capacity: size - 1 grants rank 0 one element less than it sends -- the two get XMPI_ERR_TRUNCATE, everybody
    // else succeeds, every other block is delivered, and the next call is clean
    {
      salt += (size - salt % size) % size + 1;  // (salt % size == 1: neither rank 0's row nor the last rank's column is the empty one)
      if (size == 2) salt++;
      Plan p = plan_of(rank, size, salt, 0, 0, 0);
      const bool cut = count_of(0, size - 1, salt, size) > 0;
      if (cut && rank == size - 1) p.caps[0] -= 1;
      R.fill(p.se * 8, p.re * 8);
      const int rc = xmpi_alltoallv(c, R.send, p.se, p.sc.data(), p.sd.data(), R.recv, p.re, p.caps.data(), p.rd.data(), got.data(), XMPI_I64, XMPI_ALGO_AUTO);
      const int want_rc = cut && (rank == 0 || rank == size - 1) ? XMPI_ERR_TRUNCATE : XMPI_OK;
      if (rc != want_rc) {
        fprintf(stderr, "rank %d: a pair over capacity: %d (%s), expected %d\n", rank, rc, xmpi_last_error(), want_rc);
        g_bad.fetch_add(1);
        return;
      }
      R.expect(salt, 0, 0, 0, 8, got.data(), cut && rank == size - 1 ? 0 : -1, "alltoallv, one pair over capacity");
    }
    if (!g_shared) {  // the stream form: the five arrays in device memory, read when the kernel runs
      const Plan p = plan_of(rank, size, ++salt, 3, 3, 2);
      R.fill(p.se, p.re);
      std::vector<uint64_t> rec(5 * 16, ~0ull);
      for (int j = 0; j < size; j++) {
        rec[(size_t)j] = p.sc[(size_t)j];
        rec[16 + (size_t)j] = p.sd[(size_t)j];
        rec[32 + (size_t)j] = p.caps[(size_t)j];
        rec[48 + (size_t)j] = p.rd[(size_t)j];
      }
      CHECK(xmpi_memcpy(c, R.dev, rec.data(), rec.size() * 8));
      CHECK(xmpi_alltoallv_on_stream(c, R.send, p.se, R.dev, R.dev + 16, R.recv, p.re, R.dev + 32, R.dev + 48, R.dev + 64, XMPI_U8, s));
      CHECK(xmpi_stream_sync(c, s));
      CHECK(xmpi_memcpy(c, got.data(), R.dev + 64, (size_t)size * 8));
      R.expect(salt, 3, 3, 2, 1, got.data(), -1, "alltoallv on a stream");
    }
    CHECK(xmpi_barrier(c));
  }
  if (s) CHECK(xmpi_stream_destroy(c, s));
  if (!g_shared && xmpi_get_param(c, "dsync_v_launches") == v0) {
    fprintf(stderr, "rank %d: the kernel that reads the counts never ran\n", rank);
    g_bad.fetch_add(1);
  }
  if (rank == 0 && g_bad.load() == 0)
    printf("vcoll driver: epochs %ld, launches %ld, with the counts on the device %ld\n", xmpi_get_param(c, "dsync_epoch"), xmpi_get_param(c, "dsync_launches"),
           xmpi_get_param(c, "dsync_v_launches"));
  for (void* b : {R.send, R.recv, (void*)R.dev, small_s, small_r}) (void)xmpi_free(c, b);
  CHECK(xmpi_finalize(c));
}

}  // namespace

int main(int argc, char** argv) {
  int a = 1;
  if (argc > 1 && std::string(argv[1]) == "--shared") {
    g_shared = true;
    a = 2;
  }
  const int size = argc > a ? atoi(argv[a]) : 2, rounds = argc > a + 1 ? atoi(argv[a + 1]) : 1;
  if (size < 2 || size > 16) return 2;
  setenv("XMPI_CTL_SHARE_MAPPING", "1", 1);
  setenv("DEVSIM_DEVICES", g_shared ? "1" : std::to_string(size).c_str(), 1);
  setenv("XMPI_TIMEOUT_S", "120", 0);
  setenv("XMPI_HOST_LANES", "0", 0);
  const std::string key = "devsim-vcoll-" + std::to_string((int)getpid());
  std::vector<std::thread> ranks;
  for (int r = 0; r < size; r++) ranks.emplace_back(rank_main, key, r, size, rounds);
  for (auto& t : ranks) t.join();
  if (g_bad.load()) {
    fprintf(stderr, "vcoll driver: %d failure(s)\n", g_bad.load());
    return 1;
  }
  printf("vcoll driver ok: %d ranks as threads on %d virtual device%s, %d round(s)\n", size, g_shared ? 1 : size, g_shared ? "" : "s", rounds);
  return 0;
}
