//go:build mpi_collectives_in_place

// (the build tag keeps `go vet ./...` of THIS module from compiling the file where it lies: it is a file of
// package mpi and only builds inside the reference's directory -- remove the tag line when copying it there)
//
// collectives.go -- the file a maintainer drops INTO the reference package (github.com/btracey/mpi,
// next to mpi.go) to give it the collective entry points it only stubs today
// (`//func AllReduce() {}`, mpi.go:130).  Same delegate style as mpi.go:96-159; the optional
// interface is probed on the registered backend, which is what the unused `isAllReducer`
// variable (mpi.go:69-71) was evidently reserved for.  NOT compiled here (no Go toolchain).
package mpi

import "errors"

// Collective is implemented by backends that provide collectives natively (xgmi.Backend does).
// Buffers are whatever the backend accepts as `data` in Send/Receive (xgmi.DeviceBuffer on the
// MI355X backend); op is the backend's reduction operator (xgmi.Sum, ...).
type Collective interface {
	Bcast(buf interface{}, root int) error
	Reduce(send, recv interface{}, op int, root int) error
	Allreduce(send, recv interface{}, op int) error
	Allgather(send, recv interface{}) error
	Barrier() error
}

// Personal is implemented by backends that also provide the collectives in which every rank gives every peer a DIFFERENT
// block (xgmi.Backend does): send holds Size() equal blocks, block j is for rank j.
type Personal interface {
	ReduceScatter(send, recv interface{}, op int) error
	Alltoall(send, recv interface{}) error
}

// The reduction operators a Collective / Personal backend takes as `op`: the values of xmpi_op (include/xmpi.h), which
// xgmi.Sum ... xgmi.BXor share.  OpBAnd / OpBOr / OpBXor are bitwise and defined for integer element types only.
// OpSumWide accumulates xgmi.F16 / BF16 / F8E4M3 / F8E5M2 in f32 and rounds once; for every other element type it is OpSum.
const (
	OpSum = iota
	OpProd
	OpMin
	OpMax
	OpSumWide
	OpBAnd
	OpBOr
	OpBXor
)

var errNoCollectives = errors.New("mpi: the registered implementation provides no collectives")

// Bcast replicates root's buffer on every rank.
func Bcast(buf interface{}, root int) error {
	if c, ok := mpier.(Collective); ok {
		return c.Bcast(buf, root)
	}
	return errNoCollectives
}

// Reduce folds every rank's send buffer into recv on root.
func Reduce(send, recv interface{}, op int, root int) error {
	if c, ok := mpier.(Collective); ok {
		return c.Reduce(send, recv, op, root)
	}
	return errNoCollectives
}

// Allreduce folds every rank's send buffer into recv on every rank.
func Allreduce(send, recv interface{}, op int) error {
	if c, ok := mpier.(Collective); ok {
		return c.Allreduce(send, recv, op)
	}
	return errNoCollectives
}

// Allgather concatenates every rank's send buffer, in rank order, into recv on every rank.
func Allgather(send, recv interface{}) error {
	if c, ok := mpier.(Collective); ok {
		return c.Allgather(send, recv)
	}
	return errNoCollectives
}

// ReduceScatter folds block Rank() of every rank's send buffer, in rank order, into recv (one block): the other half of Allgather.
func ReduceScatter(send, recv interface{}, op int) error {
	if c, ok := mpier.(Personal); ok {
		return c.ReduceScatter(send, recv, op)
	}
	return errNoCollectives
}

// Alltoall delivers block j of every rank's send buffer to rank j, in rank order, into recv: the exchange
// examples/helloworld/helloworld.go:53-81 performs with one Send / Receive pair per peer, as one call.
func Alltoall(send, recv interface{}) error {
	if c, ok := mpier.(Personal); ok {
		return c.Alltoall(send, recv)
	}
	return errNoCollectives
}

// PersonalV is implemented by backends that also provide the all-to-all with a count per pair.
type PersonalV interface {
	Alltoallv(send interface{}, sendcounts, sdispls []uint64, recv interface{}, recvcaps, rdispls []uint64) ([]uint64, error)
}

// Alltoallv is the exchange examples/helloworld/helloworld.go:53-81 really performs -- messages of different lengths, the receiver
// learning the length as Receive does (network.go:594-601) -- as one call; it returns the counts received.
func Alltoallv(send interface{}, sendcounts, sdispls []uint64, recv interface{}, recvcaps, rdispls []uint64) ([]uint64, error) {
	if c, ok := mpier.(PersonalV); ok {
		return c.Alltoallv(send, sendcounts, sdispls, recv, recvcaps, rdispls)
	}
	return nil, errNoCollectives
}

// Barrier blocks until every rank has called it.
func Barrier() error {
	if c, ok := mpier.(Collective); ok {
		return c.Barrier()
	}
	return errNoCollectives
}
