// alltoallv -- the exchange of the reference's own program (examples/helloworld/helloworld.go:53-81) with its own strings, as ONE
// collective.  The message a rank sends itself has another length than the one it sends a peer, and the receiver learns every
// length from the exchange (the reference's Receive re-sizes the destination to whatever arrived, network.go:594-601): an
// all-to-all with a count per pair.  The strings travel as XMPI_U8 into 64-byte slots.
//   xmpirun N alltoallv
// Prints what the reference prints.
#include <cstdio>
#include <string>
#include <vector>

#include "mpi.hpp"

int main(int argc, char** argv) {
  mpi::ParseFlags(&argc, argv);
  if (mpi::Error err = mpi::Init()) {
    fprintf(stderr, "init: %s\n", err.What().c_str());
    return 1;
  }
  const int rank = mpi::Rank(), size = mpi::Size();
  printf("Hello world, I'm node %d in a land with %d nodes\n", rank, size);
  constexpr uint64_t kSlot = 64;
  std::string out;
  std::vector<uint64_t> sendcounts, sdispls, recvcaps((size_t)size, kSlot), rdispls, recvcounts;
  for (int i = 0; i < size; i++) {
    const std::string str = i == rank ? "\"I'm just node " + std::to_string(rank) + " talking to myself\""
                                      : "\"Hello node " + std::to_string(i) + ", I'm node " + std::to_string(rank) + "\"";
    sdispls.push_back(out.size());
    sendcounts.push_back(str.size());
    rdispls.push_back((uint64_t)i * kSlot);
    out += str;
  }
  std::string in;
  int bad = 0;
  if (mpi::Error err = mpi::Alltoallv(mpi::Slice(out), sendcounts, sdispls, mpi::Into(&in), recvcaps, rdispls, &recvcounts)) {
    fprintf(stderr, "rank %d: alltoallv: %s\n", rank, err.What().c_str());
    bad++;
  } else {
    for (int i = 0; i < size; i++)
      printf("I, node %d, received a message: %s\n", rank, in.substr((size_t)i * kSlot, (size_t)recvcounts[(size_t)i]).c_str());
  }
  mpi::Barrier();
  mpi::Finalize();
  return bad ? 1 : 0;
}
