// tests/devsim/driver_personal.cpp -- xmpi_reduce_scatter and xmpi_alltoall with the ranks as THREADS of this process, every rank
// on a virtual HIP device of its own (tests/devsim), driven through the C ABI of include/xmpi.h: the personalised LL kernels
// (ll.hip ll_reduce_scatter_kernel / ll_alltoall_kernel) and the segment plans of dsync_plan.cpp (fold, push-only, meet / body / done,
// all-to-all's segment per destination) under -fsanitize=thread and, in a second build, -fsanitize=undefined
// (tests/test_personal_devsim.py builds both).  tests/devsim/driver.cpp walks the four older collectives the same way.
//
// The reference has neither collective (mpi.go:130); its own program's exchange is the all-to-all (helloworld.go:53-81).
//
// usage: driver_personal <ranks> <rounds>      --shared <ranks> <rounds>: every rank on device 0 (the ranks meet on the host)
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

// element i of the block rank `from` gives rank `to`: small integers, exactly summable in any order
inline int64_t in_i64(int from, int to, size_t i, int salt) { return (int64_t)((i * 7 + (size_t)from * 13 + (size_t)to * 29 + (size_t)salt * 5) % 1000) - 500; }

struct Rank {
  int rank, size;
  xmpi_comm* c = nullptr;
  void *send = nullptr, *recv = nullptr;
  std::vector<int64_t> host;

  void fill(size_t count, int salt) {
    host.resize((size_t)size * count);
    for (int to = 0; to < size; to++)
      for (size_t i = 0; i < count; i++) host[(size_t)to * count + i] = in_i64(rank, to, i, salt);
    (void)xmpi_memcpy(c, send, host.data(), host.size() * 8);
    (void)xmpi_memset(c, recv, 0xEE, (size_t)size * count * 8);
  }
  void expect(bool reduce, size_t count, int salt, const char* what) {
    host.resize((size_t)size * count);
    (void)xmpi_memcpy(c, host.data(), recv, (reduce ? 1 : (size_t)size) * count * 8);
    for (int from = 0; from < (reduce ? 1 : size); from++)
      for (size_t i = 0; i < count; i++) {
        int64_t want = 0;
        if (reduce)
          for (int r = 0; r < size; r++) want += in_i64(r, rank, i, salt);
        else
          want = in_i64(from, rank, i, salt);
        if (host[(size_t)from * count + i] != want) {
          fprintf(stderr, "rank %d: %s count %zu: element %zu of block %d is %lld, expected %lld\n", rank, what, count, i, from,
                  (long long)host[(size_t)from * count + i], (long long)want);
          g_bad.fetch_add(1);
          return;
        }
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
  const size_t cap = 20000;  // elements per block at most
  R.send = xmpi_malloc(c, (size_t)size * cap * 8);
  R.recv = xmpi_malloc(c, (size_t)size * cap * 8);
  if (!R.send || !R.recv) {
    g_bad.fetch_add(1);
    return;
  }
  int salt = 0;
  void* s = g_shared ? nullptr : xmpi_stream_create(c);
  for (int round = 0; round < rounds; round++) {
    // LL lines (one line, ragged, several blocks of lanes), the fold and push-only (aligned and unaligned blocks), the staged table
    for (size_t n : {(size_t)1, (size_t)33, (size_t)1025, (size_t)4096, (size_t)9001}) {
      for (int algo : {(int)XMPI_ALGO_LL, (int)XMPI_ALGO_ZCOPY, (int)XMPI_ALGO_ZPUSH, (int)XMPI_ALGO_DIRECT, (int)XMPI_ALGO_AUTO}) {
        R.fill(n, ++salt);
        CHECK(xmpi_reduce_scatter(c, R.send, R.recv, n, XMPI_I64, XMPI_SUM, algo));
        R.expect(true, n, salt, "reduce_scatter");
        if (algo == XMPI_ALGO_ZPUSH) continue;
        R.fill(n, ++salt);
        CHECK(xmpi_alltoall(c, R.send, R.recv, n, XMPI_I64, algo));
        R.expect(false, n, salt, "alltoall");
      }
    }
    // back to back without a look at the results in between: LL slots reused across kinds of collective, then the split form
    for (int k = 0; k < 6; k++) {
      R.fill(500, ++salt);
      CHECK(xmpi_alltoall(c, R.send, R.recv, 500, XMPI_I64, XMPI_ALGO_LL));
      CHECK(xmpi_allreduce(c, R.send, R.recv, 500, XMPI_I64, XMPI_SUM, XMPI_ALGO_LL));
      CHECK(xmpi_reduce_scatter(c, R.send, R.recv, 500, XMPI_I64, XMPI_SUM, XMPI_ALGO_LL));
      R.expect(true, 500, salt, "reduce_scatter behind an LL all-to-all and allreduce");
    }
    if (!g_shared) {
      CHECK(xmpi_set_param(c, "dsync_split_bytes", 1));
      R.fill(9001, ++salt);
      CHECK(xmpi_reduce_scatter(c, R.send, R.recv, 9001, XMPI_I64, XMPI_SUM, XMPI_ALGO_ZCOPY));
      R.expect(true, 9001, salt, "reduce_scatter, meet / body / done");
      R.fill(9001, ++salt);
      CHECK(xmpi_alltoall(c, R.send, R.recv, 9001, XMPI_I64, XMPI_ALGO_ZCOPY));
      R.expect(false, 9001, salt, "alltoall, meet / body / done");
      CHECK(xmpi_set_param(c, "dsync_split_bytes", 0));
      // stream-ordered, and a captured pair replayed
      R.fill(700, ++salt);
      CHECK(xmpi_alltoall_on_stream(c, R.send, R.recv, 700, XMPI_I64, s));
      CHECK(xmpi_stream_sync(c, s));
      R.expect(false, 700, salt, "alltoall on a stream");
      void* g = nullptr;
      CHECK(xmpi_graph_begin(c, s));
      CHECK(xmpi_reduce_scatter_on_stream(c, R.send, R.recv, 700, XMPI_I64, XMPI_SUM, s));
      CHECK(xmpi_graph_end(c, s, &g));
      for (int k = 0; k < 3; k++) {
        CHECK(xmpi_barrier(c));  // (a replay reads the peers' send buffers: nobody refills one under it)
        R.fill(700, ++salt);
        CHECK(xmpi_barrier(c));
        CHECK(xmpi_graph_launch(c, g, s));
        CHECK(xmpi_stream_sync(c, s));
        R.expect(true, 700, salt, "reduce_scatter, graph replay");
      }
      CHECK(xmpi_graph_destroy(c, g));
    }
    CHECK(xmpi_barrier(c));
  }
  if (s) CHECK(xmpi_stream_destroy(c, s));
  if (rank == 0 && g_bad.load() == 0)
    printf("personal driver: epochs %ld, launches %ld, split %ld, LL %ld\n", xmpi_get_param(c, "dsync_epoch"), xmpi_get_param(c, "dsync_launches"),
           xmpi_get_param(c, "dsync_split_launches"), xmpi_get_param(c, "dsync_ll_launches"));
  (void)xmpi_free(c, R.send);
  (void)xmpi_free(c, R.recv);
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
  const std::string key = "devsim-personal-" + std::to_string((int)getpid());
  std::vector<std::thread> ranks;
  for (int r = 0; r < size; r++) ranks.emplace_back(rank_main, key, r, size, rounds);
  for (auto& t : ranks) t.join();
  if (g_bad.load()) {
    fprintf(stderr, "personal driver: %d failure(s)\n", g_bad.load());
    return 1;
  }
  printf("personal driver ok: %d ranks as threads on %d virtual device%s, %d round(s)\n", size, g_shared ? 1 : size, g_shared ? "" : "s", rounds);
  return 0;
}
