// mpi::Network with XMPI_BAND / XMPI_BOR / XMPI_BXOR: three ranks as three objects in one process (threads), loopback TCP.
// Allreduce and Reduce of int32 and int64 by each operator against a host loop; float64 refused before anything is exchanged.
//   tcp_bitop_check [first port]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "network.hpp"

namespace {

constexpr int kRanks = 3;
constexpr size_t kCount = 1003;

uint64_t mix(uint64_t x) {  // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// dense words for AND, sparse ones for OR: the result is neither all zeros nor all ones
template <typename T>
std::vector<T> input(int rank, xmpi_op op) {
  std::vector<T> v(kCount);
  for (size_t i = 0; i < kCount; i++) {
    const uint64_t a = mix(1000 * (uint64_t)rank + i), b = mix(a);
    v[i] = (T)(op == XMPI_BAND ? (a | b) : op == XMPI_BOR ? (a & b) : a);
  }
  return v;
}

template <typename T>
T fold(T a, T b, xmpi_op op) {
  return op == XMPI_BAND ? (T)(a & b) : op == XMPI_BOR ? (T)(a | b) : (T)(a ^ b);
}

template <typename T>
int check_type(mpi::Network* net, const char* name) {
  int bad = 0;
  for (xmpi_op op : {XMPI_BAND, XMPI_BOR, XMPI_BXOR}) {
    std::vector<std::vector<T>> in(kRanks), all(kRanks), red(kRanks);
    std::vector<T> want;
    for (int r = 0; r < kRanks; r++) {
      in[r] = input<T>(r, op);
      if (r == 0) want = in[0];
      else
        for (size_t i = 0; i < kCount; i++) want[i] = fold(want[i], in[r][i], op);
    }
    size_t set = 0, flipped = 0;
    for (size_t i = 0; i < kCount; i++) {
      set += want[i] != 0 && want[i] != (T)-1;
      flipped += want[i] != in[0][i];
    }
    if (set < kCount / 2 || flipped < kCount / 2) {
      printf("FAILED: %s op %d: the expectation is a constant or rank 0's input\n", name, (int)op);
      bad++;
    }
    std::vector<mpi::Error> ea(kRanks), er(kRanks);
    std::vector<std::thread> ts;
    for (int r = 0; r < kRanks; r++)
      ts.emplace_back([&, r] {
        ea[r] = net[r].Allreduce(mpi::Slice(in[r]), mpi::Into(&all[r]), op);
        er[r] = net[r].Reduce(mpi::Slice(in[r]), mpi::Into(&red[r]), op, kRanks - 1);
      });
    for (auto& t : ts) t.join();
    for (int r = 0; r < kRanks; r++) {
      if (ea[r] || all[r] != want) {
        printf("FAILED: %s allreduce op %d on rank %d: %s\n", name, (int)op, r, ea[r] ? ea[r].What().c_str() : "wrong bits");
        bad++;
      }
      if (er[r] || (r == kRanks - 1 && red[r] != want)) {
        printf("FAILED: %s reduce op %d on rank %d: %s\n", name, (int)op, r, er[r] ? er[r].What().c_str() : "wrong bits");
        bad++;
      }
    }
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const int port = argc > 1 ? atoi(argv[1]) : 8171;
  std::vector<std::string> addrs;
  for (int r = 0; r < kRanks; r++) addrs.push_back(":" + std::to_string(port + r));
  mpi::Network net[kRanks];
  std::vector<mpi::Error> e(kRanks);
  {
    std::vector<std::thread> ts;
    for (int r = 0; r < kRanks; r++)
      ts.emplace_back([&, r] {
        net[r].Addr = addrs[r];
        net[r].Addrs = addrs;
        net[r].Timeout = 20;
        net[r].NetProto = "tcp";
        e[r] = net[r].Init();
      });
    for (auto& t : ts) t.join();
  }
  int bad = 0;
  for (int r = 0; r < kRanks; r++)
    if (e[r] || net[r].Rank() != r || net[r].Size() != kRanks) {
      printf("FAILED: Init of rank %d: %s\n", r, e[r].What().c_str());
      bad++;
    }
  if (bad) return 1;
  bad += check_type<int32_t>(net, "int32");
  bad += check_type<int64_t>(net, "int64");
  // float64 (and float32) with a bitwise operator: XMPI_ERR_ARG from the arguments -- no rank sends anything, so a rank that calls
  // ALONE returns (it would wait for its peers if the refusal came after the exchange)
  for (xmpi_op op : {XMPI_BAND, XMPI_BOR, XMPI_BXOR}) {
    std::vector<double> d(kCount, 1.5), dg;
    std::vector<float> f(kCount, 1.5f), fg;
    const mpi::Error a = net[1].Allreduce(mpi::Slice(d), mpi::Into(&dg), op), b = net[0].Reduce(mpi::Slice(d), mpi::Into(&dg), op, 0),
                     c = net[2].Allreduce(mpi::Slice(f), mpi::Into(&fg), op);
    for (const mpi::Error* x : {&a, &b, &c})
      if (x->Code() != XMPI_ERR_ARG || x->What().find("integer type") == std::string::npos) {
        printf("FAILED: a float type with op %d: code %d, \"%s\"\n", (int)op, x->Code(), x->What().c_str());
        bad++;
      }
  }
  {  // an operator that does not exist is still refused, and the backend is usable after all of this
    std::vector<int32_t> v(kCount, 1), g;
    if (net[0].Allreduce(mpi::Slice(v), mpi::Into(&g), (xmpi_op)8).Code() != XMPI_ERR_ARG) {
      printf("FAILED: operator 8 was not refused\n");
      bad++;
    }
    std::vector<std::vector<int32_t>> out(kRanks);
    std::vector<std::thread> ts;
    for (int r = 0; r < kRanks; r++) ts.emplace_back([&, r] { e[r] = net[r].Allreduce(mpi::Slice(v), mpi::Into(&out[r]), XMPI_SUM); });
    for (auto& t : ts) t.join();
    for (int r = 0; r < kRanks; r++)
      if (e[r] || out[r] != std::vector<int32_t>(kCount, kRanks)) {
        printf("FAILED: XMPI_SUM after the refusals on rank %d\n", r);
        bad++;
      }
  }
  {
    std::vector<std::thread> ts;
    for (int r = 0; r < kRanks; r++) ts.emplace_back([&, r] { net[r].Finalize(); });
    for (auto& t : ts) t.join();
  }
  printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
