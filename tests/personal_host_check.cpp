// Host-logic checks of mpi::ReduceScatter / mpi::Alltoall in the C++ mirror of package mpi (no GPU needed): the package-level
// functions probe the registered backend (cf. `isAllReducer`, mpi.go:69-71; the collectives themselves are a stub upstream,
// mpi.go:130), a backend with the four older collectives answers "unsupported by this backend" for the two new ones, and the xGMI
// backend refuses a send buffer that is not one block per rank before it calls the library.  Prints "ok" and exits 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpi.hpp"

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
      return 1;                                               \
    }                                                         \
  } while (0)

// a backend with the four older collectives only
struct Older : mpi::Interface, mpi::Collective {
  int gathers = 0;
  mpi::Error Init() override { return mpi::Error(); }
  void Finalize() override {}
  int Rank() override { return 1; }
  int Size() override { return 4; }
  mpi::Error Send(const mpi::Data&, int, int) override { return mpi::Error(); }
  mpi::Error Receive(mpi::Data, int, int) override { return mpi::Error(); }
  mpi::Error Bcast(mpi::Data, int) override { return mpi::Error(); }
  mpi::Error Reduce(const mpi::Data&, mpi::Data, xmpi_op, int) override { return mpi::Error(); }
  mpi::Error Allreduce(const mpi::Data&, mpi::Data, xmpi_op) override { return mpi::Error(); }
  mpi::Error Allgather(const mpi::Data&, mpi::Data) override { gathers++; return mpi::Error(); }
  mpi::Error Barrier() override { return mpi::Error(); }
};

int main() {
  std::vector<float> send(12, 1.0f), recv;
  // the default backend, not initialised: no ranks, so no buffer is "one block per rank" -- an argument error, no call into the library
  mpi::Error e = mpi::Alltoall(mpi::Slice(send), mpi::Into(&recv));
  CHECK(e && e.Code() == XMPI_ERR_ARG && e.What().find("one block per rank") != std::string::npos);
  e = mpi::ReduceScatter(mpi::Slice(send), mpi::Into(&recv));
  CHECK(e && e.Code() == XMPI_ERR_ARG && e.What().find("mpi reduce_scatter") != std::string::npos);
  CHECK(recv.empty());
  mpi::XGMI x;
  e = x.AlltoallOnStream(mpi::Slice(send), mpi::Span(send.data(), 12), nullptr);
  CHECK(e && e.Code() == XMPI_ERR_ARG);
  e = x.ReduceScatterOnStream(mpi::Slice(send), mpi::Span(send.data(), 3), XMPI_SUM, nullptr);
  CHECK(e && e.Code() == XMPI_ERR_ARG);

  Older older;
  mpi::Register(&older);
  CHECK(!mpi::Allgather(mpi::Slice(send), mpi::Into(&recv)) && older.gathers == 1);
  e = mpi::ReduceScatter(mpi::Slice(send), mpi::Into(&recv), XMPI_MAX);
  CHECK(e && e.Code() == XMPI_ERR_UNSUPPORTED && e.What().find("unsupported by this backend") != std::string::npos);
  e = mpi::Alltoall(mpi::Slice(send), mpi::Into(&recv));
  CHECK(e && e.Code() == XMPI_ERR_UNSUPPORTED && e.What().find("mpi alltoall") != std::string::npos);
  printf("ok\n");
  return 0;
}
