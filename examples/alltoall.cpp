// alltoall -- the exchange of the reference's own program (examples/helloworld/helloworld.go:53-81: every rank sends a distinct
// message to every rank, there as N-1 Send / Receive pairs per rank) as ONE collective on host slices, then a reduce-scatter
// of the same blocks checked against a host sum in rank order.  The reference stubs its collectives (mpi.go:130).
//   xmpirun N alltoall [elements per block]
// Every rank prints `ok`; a mismatch is reported and the exit code is non-zero.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mpi.hpp"

// what rank `from` has to say to rank `to`, element i
static double word(int from, int to, size_t i) { return (double)(from * 1000 + to) + (double)(i % 13) * 0.25; }

int main(int argc, char** argv) {
  mpi::ParseFlags(&argc, argv);
  if (mpi::Error err = mpi::Init()) {
    fprintf(stderr, "init: %s\n", err.What().c_str());
    return 1;
  }
  const int rank = mpi::Rank(), size = mpi::Size();
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 1000;
  std::vector<double> out((size_t)size * n), in, sum;
  for (int to = 0; to < size; to++)
    for (size_t i = 0; i < n; i++) out[(size_t)to * n + i] = word(rank, to, i);
  int bad = 0;
  if (mpi::Error err = mpi::Alltoall(mpi::Slice(out), mpi::Into(&in))) {
    fprintf(stderr, "rank %d: alltoall: %s\n", rank, err.What().c_str());
    bad++;
  } else {
    for (int from = 0; from < size && !bad; from++)
      for (size_t i = 0; i < n; i++)
        if (in.size() != out.size() || in[(size_t)from * n + i] != word(from, rank, i)) {
          fprintf(stderr, "rank %d: alltoall: element %zu of rank %d's block differs\n", rank, i, from);
          bad++;
          break;
        }
  }
  if (mpi::Error err = mpi::ReduceScatter(mpi::Slice(out), mpi::Into(&sum), XMPI_SUM)) {
    fprintf(stderr, "rank %d: reduce_scatter: %s\n", rank, err.What().c_str());
    bad++;
  } else {
    for (size_t i = 0; i < n; i++) {
      double want = word(0, rank, i);  // the host sum a reference user computes after receiving everything, in rank order
      for (int from = 1; from < size; from++) want += word(from, rank, i);
      if (sum.size() != n || sum[i] != want) {
        fprintf(stderr, "rank %d: reduce_scatter: element %zu is %.17g, the rank-order sum %.17g\n", rank, i, sum.size() == n ? sum[i] : 0.0, want);
        bad++;
        break;
      }
    }
  }
  mpi::Barrier();
  mpi::Finalize();
  if (bad) return 1;
  printf("rank %d of %d: ok\n", rank, size);
  return 0;
}
