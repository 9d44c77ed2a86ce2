"""Scenarios of the collectives in which every rank gives every peer a DIFFERENT block: xmpi_reduce_scatter and xmpi_alltoall.
Each function runs on ONE rank (a process or a thread, tests/personal_worker.py) and checks its own results, bit for bit:
all-to-all against a numpy re-slicing of the ranks' inputs, reduce-scatter against the CPU oracle's rank-order fold
(oracle_reduce_ranks) over block `me` of every rank's input.  No tolerance anywhere: both collectives are exact."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

from mpi_amd import xmpi
from oracle import oracle
from tests import hard_inputs as hi

RS, A2A = "reduce_scatter", "alltoall"
DTYPES = (xmpi.U8, xmpi.I32, xmpi.I64, xmpi.F16, xmpi.F32, xmpi.F64, xmpi.BF16)
OPS = (xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX)
COUNTS = (1, 3, 17, 1000, 4099, 65536 + 5)  # per block: one element, ragged lines, below / above the LL limit, unaligned blocks
RS_ALGOS = (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_DIRECT)
A2A_ALGOS = (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_LL, xmpi.ALGO_DIRECT)
GUARD = 64  # bytes behind a host receive slice that must stay as they were
PAD = 256   # bytes in front of and behind a device buffer that must stay as they were (a block's alignment: the buffer keeps it)
SEND_PAD, RECV_PAD = 0x5E, 0xC7  # different: pad copied onto pad would show

_inputs = {}  # (dtype, elements, seed) -> the oracle's fill: computed once, shared by the cases, never written


def rank_input(dtype: int, n: int, seed: int) -> np.ndarray:
    key = (dtype, n, seed)
    if key not in _inputs:
        a = oracle.fill(n, dtype, xmpi.PAT_SIGNED if dtype != xmpi.U8 else xmpi.PAT_UNIFORM, seed)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def expected(coll: str, me: int, size: int, dtype: int, count: int, op: int, seed: int) -> np.ndarray:
    blocks = [rank_input(dtype, size * count, seed + r)[me * count:(me + 1) * count] for r in range(size)]
    if coll == A2A:
        return np.concatenate(blocks)
    return oracle.reduce_ranks(blocks, dtype, op)


def _hip_runtime():
    return ctypes.CDLL(os.environ.get("XMPI_DEVSIM_LIB") or "libamdhip64.so")


def _call(comm, coll, send, recv, count, dtype, op, algo, stream):
    if stream is not None:
        if coll == RS:
            comm.reduce_scatter_on_stream(send, recv, count, dtype, op, stream)
        else:
            comm.alltoall_on_stream(send, recv, count, dtype, stream)
        comm.stream_sync(stream)
    elif coll == RS:
        comm.reduce_scatter(send, recv, count, dtype, op, algo)
    else:
        comm.alltoall(send, recv, count, dtype, algo)


def personal_case(comm, coll, dtype, count, algo=xmpi.ALGO_AUTO, op=xmpi.SUM, seed=4000, mem="registered", stream=None):
    """one call, checked; mem: registered (xmpi_malloc) | host (numpy slices) | foreign (hipMalloc, never registered)"""
    me, size = comm.rank(), comm.size()
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    mine = rank_input(dtype, size * count, seed + me)
    want = expected(coll, me, size, dtype, count, op, seed)
    sb, rb = size * count * es, want.nbytes
    what = f"{coll} {xmpi.DTYPE_NAME[dtype]} count={count} algo={algo} op={op} mem={mem} stream={stream is not None} rank {me}/{size}"
    if mem == "host":
        send = mine.copy()
        recv = np.full(rb + GUARD, 0xA5, dtype=np.uint8)
        _call(comm, coll, send, recv[:rb].view(npdt), count, dtype, op, algo, stream)
        assert recv[:rb].tobytes() == want.tobytes(), f"{what}: differs from the expectation"
        assert np.all(recv[rb:] == 0xA5), f"{what}: wrote past the receive buffer"
        assert send.tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
        return
    # both buffers inside frames: PAD bytes in front and behind, the send frame's and the receive frame's of different bytes
    if mem == "foreign":
        hip = _hip_runtime()
        s, r = ctypes.c_void_p(0), ctypes.c_void_p(0)
        comm.sync()
        assert hip.hipMalloc(ctypes.byref(s), ctypes.c_size_t(sb + 2 * PAD)) == 0 and hip.hipMalloc(ctypes.byref(r), ctypes.c_size_t(rb + 2 * PAD)) == 0
        sf, rf = s.value, r.value
    else:
        send, recv = comm.alloc(sb + 2 * PAD), comm.alloc(rb + 2 * PAD)
        sf, rf = send.ptr, recv.ptr
    sp, rp = sf + PAD, rf + PAD
    pad = np.full(PAD, RECV_PAD, dtype=np.uint8)
    wantd = comm.alloc(rb + 2 * PAD).upload(np.concatenate([pad, want.view(np.uint8), pad]))
    simage = np.concatenate([np.full(PAD, SEND_PAD, dtype=np.uint8), mine.view(np.uint8), np.full(PAD, SEND_PAD, dtype=np.uint8)])
    comm.memcpy(sf, simage.ctypes.data, sb + 2 * PAD)
    comm.memset(rf, RECV_PAD, rb + 2 * PAD)
    comm.memset(rp, 0xA5, rb)
    _call(comm, coll, sp, rp, count, dtype, op, algo, stream)
    bad = comm.count_mismatch(rf, wantd, rb + 2 * PAD)  # (the whole buffer and the bytes in front of and behind it, on the device)
    if bad:
        got = np.empty(rb + 2 * PAD, dtype=np.uint8)
        comm.memcpy(got.ctypes.data, rf, rb + 2 * PAD)
        idx = np.nonzero(got != np.concatenate([pad, want.view(np.uint8), pad]))[0]
        raise AssertionError(f"{what}: {bad} bytes differ, first at byte {int(idx[0]) - PAD} of {rb} (negative: in front of the receive buffer)")
    back = np.empty(sb + 2 * PAD, dtype=np.uint8)
    comm.memcpy(back.ctypes.data, sf, sb + 2 * PAD)
    assert back[PAD:PAD + sb].tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
    assert back.tobytes() == simage.tobytes(), f"{what}: bytes in front of or behind the send buffer were written"
    wantd.free()
    if mem == "foreign":
        comm.barrier()
        assert hip.hipFree(s) == 0 and hip.hipFree(r) == 0
    else:
        send.free()
        recv.free()


def sc_algos(comm, args):
    """every algorithm name at a count below the LL limit, an unaligned one above it and -- the meet / body / done form -- one
    large enough to be split; every name gives the same bits (they are all compared with the one expectation)"""
    counts = args.get("counts", [5, 1000, 8209])
    for count in counts:
        for algo in RS_ALGOS:
            personal_case(comm, RS, xmpi.F32, count, algo, xmpi.SUM)
        for algo in A2A_ALGOS:
            personal_case(comm, A2A, xmpi.F32, count, algo)
    # meet / body / done, forced by size (dsync_split_bytes) as for the allreduce; one kernel when it is 0
    big = args.get("split_count", 40000)
    for split in (1, 0):
        comm.set_param("dsync_split_bytes", split)
        for algo in (xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH):
            personal_case(comm, RS, xmpi.F64, big, algo, xmpi.SUM)
        personal_case(comm, A2A, xmpi.I32, big + 3, xmpi.ALGO_ZCOPY)
    if comm.get_param("dsync"):
        assert comm.get_param("dsync_split_launches") > 0, "the meet / body / done form never ran"


def sc_sweep(comm, args):
    """all 7 dtypes x 4 operations at every count, AUTO: LL lines up to ll_bytes per block, the fold above"""
    counts = args.get("counts", list(COUNTS))
    dtypes = args.get("dtypes", list(DTYPES))
    ll0 = comm.get_param("dsync_ll_launches")
    for dtype in dtypes:
        for count in counts:
            for op in OPS:
                personal_case(comm, RS, dtype, count, xmpi.ALGO_AUTO, op, seed=4100 + 7 * op)
            personal_case(comm, A2A, dtype, count, xmpi.ALGO_AUTO, seed=4200)
    if comm.get_param("dsync") and min(counts) * 8 <= comm.get_param("ll_bytes"):
        assert comm.get_param("dsync_ll_launches") > ll0, "AUTO never took the LL lines for a small block"


def sc_memory(comm, args):
    """host slices, device memory nobody registered, the stream-ordered forms"""
    for count in (1, 1000, 20001):
        for mem in ("host", "foreign"):
            for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_LL):
                personal_case(comm, RS, xmpi.F32, count, algo, xmpi.SUM, mem=mem)
                personal_case(comm, A2A, xmpi.I64, count, algo, mem=mem)
        personal_case(comm, RS, xmpi.BF16, count, xmpi.ALGO_ZPUSH, xmpi.MAX, mem="host")
    st = comm.stream_create()
    for count in (3, 1000, 20001):
        personal_case(comm, RS, xmpi.F64, count, op=xmpi.SUM, stream=st)
        personal_case(comm, A2A, xmpi.F16, count, stream=st)
        if comm.get_param("dsync"):  # (ranks that meet on the host: the stream-ordered forms take registered memory)
            personal_case(comm, A2A, xmpi.I32, count, stream=st, mem="foreign")
    comm.stream_destroy(st)


def sc_graph(comm, args):
    """a captured graph of {alltoall, reduce_scatter, allreduce}, replayed 3 times with new inputs each time"""
    me, size = comm.rank(), comm.size()
    for count in (100, 9000):  # LL lines / the fold
        n = size * count
        a, b, c, d = comm.alloc(n * 8), comm.alloc(n * 8), comm.alloc(count * 8), comm.alloc(count * 8)
        st = comm.stream_create()
        # (everything mapped before the capture)
        comm.alltoall_on_stream(a, b, count, xmpi.I64, st)
        comm.reduce_scatter_on_stream(b, c, count, xmpi.I64, xmpi.SUM, st)
        comm.allreduce_on_stream(c, d, count, xmpi.I64, xmpi.MAX, st)
        comm.stream_sync(st)
        comm.graph_begin(st)
        comm.alltoall_on_stream(a, b, count, xmpi.I64, st)
        comm.reduce_scatter_on_stream(b, c, count, xmpi.I64, xmpi.SUM, st)
        comm.allreduce_on_stream(c, d, count, xmpi.I64, xmpi.MAX, st)
        graph = comm.graph_end(st)
        for rep in range(3):
            ins = [rank_input(xmpi.I64, n, 4300 + 10 * rep + r) for r in range(size)]
            a.upload(ins[me])
            comm.barrier()  # (nobody's replay stores into a buffer its owner is still filling)
            comm.graph_launch(graph, st)
            comm.stream_sync(st)
            # what rank q holds after the all-to-all, its reduce-scatter, then the maximum over the ranks
            bq = [np.concatenate([ins[r][q * count:(q + 1) * count] for r in range(size)]) for q in range(size)]
            cq = [oracle.reduce_ranks([bq[r][q * count:(q + 1) * count] for r in range(size)], xmpi.I64, xmpi.SUM) for q in range(size)]
            want = oracle.reduce_ranks(cq, xmpi.I64, xmpi.MAX)
            assert b.download(np.int64, n).tobytes() == bq[me].tobytes(), f"graph replay {rep}: alltoall count={count}"
            assert c.download(np.int64, count).tobytes() == cq[me].tobytes(), f"graph replay {rep}: reduce_scatter count={count}"
            assert d.download(np.int64, count).tobytes() == want.tobytes(), f"graph replay {rep}: allreduce count={count}"
            comm.barrier()
        comm.graph_destroy(graph)
        comm.stream_destroy(st)
        for x in (a, b, c, d):
            x.free()


def sc_parity(comm, args):
    """50 calls back to back, no barrier between them, alternating LL all-to-all / LL allreduce / fold reduce-scatter / LL
    reduce-scatter: the LL slots' parity is reused across kinds of collective (kernels.h: a rank completes a call only after every
    peer has started it -- for the personalised forms by their data alone)"""
    me, size = comm.rank(), comm.size()
    count = args.get("count", 257)
    n = size * count
    send, a2a, ar, rs_fold, rs_ll = comm.alloc(n * 4), comm.alloc(n * 4), comm.alloc(count * 4), comm.alloc(count * 4), comm.alloc(count * 4)
    wants = {}
    for k in range(50):
        seed = 4400 + (k % 5) * 16
        ins = [rank_input(xmpi.I32, n, seed + r) for r in range(size)]
        send.upload(ins[me])
        kind = k % 4
        if kind == 0:
            comm.alltoall(send, a2a, count, xmpi.I32, xmpi.ALGO_LL)
            got, want = a2a.download(np.int32, n), expected(A2A, me, size, xmpi.I32, count, xmpi.SUM, seed)
        elif kind == 1:
            comm.allreduce(send, ar, count, xmpi.I32, xmpi.SUM, xmpi.ALGO_LL)
            got, want = ar.download(np.int32, count), oracle.reduce_ranks([x[:count] for x in ins], xmpi.I32, xmpi.SUM)
        elif kind == 2:
            comm.reduce_scatter(send, rs_fold, count, xmpi.I32, xmpi.SUM, xmpi.ALGO_ZCOPY)
            got, want = rs_fold.download(np.int32, count), expected(RS, me, size, xmpi.I32, count, xmpi.SUM, seed)
        else:
            comm.reduce_scatter(send, rs_ll, count, xmpi.I32, xmpi.MIN, xmpi.ALGO_LL)
            got, want = rs_ll.download(np.int32, count), expected(RS, me, size, xmpi.I32, count, xmpi.MIN, seed)
        assert got.tobytes() == want.tobytes(), f"call {k} (kind {kind}) of the back-to-back sequence differs, rank {me}/{size}"
    for x in (send, a2a, ar, rs_fold, rs_ll):
        x.free()


def sc_layout(comm, args):
    """the other layouts -- rank threads of one process, XMPI_DSYNC=0, XMPI_ZERO_COPY=0 (the staged tables), 9 and 12 ranks on 8
    devices: every name, a few dtypes and operations, ragged counts; the same bits as everywhere else"""
    # (XMPI_ZERO_COPY=0: a zero-copy NAME still asks for the zero-copy fold; the staged tables are what AUTO and DIRECT run there)
    staged = (xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT)
    for count in args.get("counts", [1, 17, 1000, 4099]):
        for algo in (staged if args.get("expect_staged") else RS_ALGOS):
            personal_case(comm, RS, xmpi.F32, count, algo, xmpi.SUM)
        for algo in (staged if args.get("expect_staged") else A2A_ALGOS):
            personal_case(comm, A2A, xmpi.I64, count, algo)
        personal_case(comm, RS, xmpi.BF16, count, xmpi.ALGO_AUTO, xmpi.PROD)
        personal_case(comm, RS, xmpi.U8, count, xmpi.ALGO_DIRECT, xmpi.MAX)
        personal_case(comm, A2A, xmpi.U8, count, xmpi.ALGO_DIRECT)
    personal_case(comm, RS, xmpi.F64, 1000, xmpi.ALGO_AUTO, xmpi.SUM, mem="host")
    personal_case(comm, A2A, xmpi.F16, 1000, xmpi.ALGO_AUTO, mem="host")
    if args.get("expect_staged"):
        assert comm.get_param("zc_seq") == 0 and comm.get_param("dsync_launches") == 0, "the staged tables were not what ran"
    if args.get("expect_host_fold"):
        assert comm.get_param("zc_seq") > 0 and comm.get_param("dsync_launches") == 0, "the host-rendezvous fold was not what ran"


_hard_blocks = {}  # (dtype, count, seed, size, op == PROD) -> block q of rank r's send buffer, for every q and r: computed once, never written


def hard_blocks(dtype: int, count: int, seed: int, size: int, op: int):
    """tests/hard_inputs.py data for the personalised collectives: block q of every rank's send buffer is one `special` job of its
    own (seed + 100 q) -- all 256 ordered pairs of specials meet in EVERY rank's result, not only in rank 0's -- and dense(spread 1)
    for a product"""
    key = (dtype, count, seed, size, op == xmpi.PROD)
    if key not in _hard_blocks:
        blocks = [hi.rank_inputs(dtype, count, seed + 100 * q, size, op) for q in range(size)]  # [q][r]
        for row in blocks:
            for x in row:
                x.setflags(write=False)
        _hard_blocks[key] = blocks
    return _hard_blocks[key]


def hard_personal_case(comm, coll, dtype, count, algo, op=xmpi.SUM, seed=8000):
    """one reduce-scatter (against oracle_reduce_ranks over block `me` of every rank's input, under same_floats) or all-to-all (byte
    for byte: a copy touches no bit, a signalling NaN's payload and -0 included) of that data"""
    me, size = comm.rank(), comm.size()
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    blocks = hard_blocks(dtype, count, seed, size, op)
    mine = np.concatenate([blocks[q][me] for q in range(size)])
    what = f"{coll} of hard inputs {xmpi.DTYPE_NAME[dtype]} count={count} algo={algo} op={op} rank {me}/{size}"
    rb = (count if coll == RS else size * count) * es
    sb = size * count * es
    send, recv = comm.alloc(sb + 2 * PAD), comm.alloc(rb + 2 * PAD)
    comm.memset(send, SEND_PAD, sb + 2 * PAD)
    send.upload(mine, PAD)
    comm.memset(recv, RECV_PAD, rb + 2 * PAD)
    comm.memset(recv.at(PAD), 0xA5, rb)
    _call(comm, coll, send.at(PAD), recv.at(PAD), count, dtype, op, algo, None)
    got = recv.download(npdt, rb // es, byte_offset=PAD)
    if coll == RS:
        hi.same_floats(got, oracle.reduce_ranks(blocks[me], dtype, op), dtype, op, what)
    else:
        assert got.tobytes() == b"".join(blocks[me][r].tobytes() for r in range(size)), f"{what}: bits changed on the way"
    assert np.all(recv.download(np.uint8, PAD, byte_offset=PAD + rb) == RECV_PAD), f"{what}: wrote past the receive buffer"
    assert np.all(recv.download(np.uint8, PAD) == RECV_PAD), f"{what}: wrote in front of the receive buffer"
    assert send.download(npdt, size * count, byte_offset=PAD).tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
    assert np.all(send.download(np.uint8, PAD) == SEND_PAD) and np.all(send.download(np.uint8, PAD, byte_offset=PAD + sb) == SEND_PAD), \
        f"{what}: bytes in front of or behind the send buffer were written"
    send.free()
    recv.free()


def sc_hard(comm, args):
    """reduce-scatter's rank-order claim where it can be seen (tests/hard_inputs.py): the four float types x {SUM, MIN, MAX} on
    `special` data and PROD on dense(spread 1) data, 1003 elements per block (LL lines for every type, ragged) and 8209 (above
    ll_bytes: packets, a tail, unaligned blocks), by every name, one kernel and meet / body / done -- the counters say which ran;
    and all-to-all of special f32 / f16 data by every name, byte for byte"""
    me, size = comm.rank(), comm.size()
    counts = args.get("counts", [1003, 8209])
    staged = bool(args.get("expect_staged"))
    dsync = comm.get_param("dsync") == 1
    names = ("zc_seq", "dsync_launches", "dsync_ll_launches", "dsync_split_launches", "ll_bytes")
    counters = lambda: {k: comm.get_param(k) for k in names}
    maxb = comm.get_param("ll_max_bytes")
    split0 = comm.get_param("dsync_split_bytes")

    def ran(algo, split, unit, b, a):
        d = {k: a[k] - b[k] for k in names}
        if staged:
            return a["zc_seq"] == 0 and a["dsync_launches"] == 0
        if not dsync:  # the host rendezvous (DIRECT: the staged table)
            return a["dsync_launches"] == 0 and d["zc_seq"] == (0 if algo == xmpi.ALGO_DIRECT else 1)
        if algo == xmpi.ALGO_DIRECT:
            return d["dsync_launches"] == 0 and d["dsync_ll_launches"] == 0
        if (algo == xmpi.ALGO_LL and unit <= maxb) or (algo == xmpi.ALGO_AUTO and unit <= b["ll_bytes"]):
            return d["dsync_ll_launches"] == 1 and d["dsync_split_launches"] == 0
        if algo == xmpi.ALGO_ZPUSH:
            return d["dsync_ll_launches"] == 0 and d["dsync_launches"] >= 1
        return d["dsync_ll_launches"] == 0 and ((d["dsync_split_launches"], d["dsync_launches"]) == ((1, 3) if split else (0, 1)))

    n = 0
    for split in (1, 0) if dsync else (None,):
        if split is not None:
            comm.set_param("dsync_split_bytes", split)
        for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT) if staged else RS_ALGOS:
            for dtype in hi.FLOATS:
                for op in OPS:
                    for count in counts:
                        before = counters()
                        hard_personal_case(comm, RS, dtype, count, algo, op)
                        after = counters()
                        n += 1
                        assert ran(algo, split, count * xmpi.DTYPE_SIZE[dtype], before, after), \
                            f"reduce_scatter algo={algo} split={split} {xmpi.DTYPE_NAME[dtype]} count={count}: another form ran, counters {before} -> {after}"
        for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT) if staged else A2A_ALGOS:
            for dtype in (xmpi.F32, xmpi.F16):
                for count in counts:
                    hard_personal_case(comm, A2A, dtype, count, algo)
    if dsync:
        comm.set_param("dsync_split_bytes", split0)
    if me == 0:
        print(f"personal hard: {n} reduce-scatters checked, each with its form confirmed by the counters")


def sc_mismatch(comm, args):
    """ranks in different calls -- an all-to-all against a reduce-scatter over the same bytes, above the LL limit: every rank gets
    XMPI_ERR_ARG at once, nothing is moved.  (Virtual devices only.)"""
    import time
    me, size = comm.rank(), comm.size()
    count = 3000  # x 8 bytes = 24000 per block ...
    a, b = comm.alloc(size * count * 8), comm.alloc(size * count * 8)
    comm.fill(a, size * count, xmpi.I64, xmpi.PAT_INDEX, me)
    personal_case(comm, A2A, xmpi.I64, count, xmpi.ALGO_ZCOPY)  # (everything mapped)
    comm.memset(b, 0x5A, size * count * 8)
    comm.set_param("ll_bytes", 0)  # ... so AUTO would take the fold too; ZCOPY names it
    t0 = time.time()
    try:
        if me == size - 1:
            comm.reduce_scatter(a, b, count, xmpi.I64, xmpi.SUM, xmpi.ALGO_ZCOPY)
        else:
            comm.alltoall(a, b, count, xmpi.I64, xmpi.ALGO_ZCOPY)
    except xmpi.XmpiError as e:
        took = time.time() - t0
        assert e.code == xmpi.ERR_ARG and "not in the same call" in str(e), e
        assert took < 5, f"the error took {took:.1f} s -- somebody waited for a clock"
        assert np.all(b.download(np.uint8, size * count * 8) == 0x5A), "a peer wrote into this rank's buffer although the calls differed"
        print(f"rank {me}/{size} personal mismatch: ok (error after {took * 1e3:.0f} ms)")
        sys.stdout.flush()
        os._exit(0)  # (the job is aborted: no finalize barrier)
    raise AssertionError("ranks in different calls returned without an error")


def sc_fullsize(comm, args):
    """8 ranks x 32 MiB per block, f32: both collectives by the fold, the whole buffers checked on the device"""
    me, size = comm.rank(), comm.size()
    count = args.get("count", 8 << 20)
    n = size * count
    send, recv, small, want = comm.alloc(n * 4), comm.alloc(n * 4), comm.alloc(count * 4), comm.alloc(n * 4)
    # rank r's block q = oracle_fill(seed 5000 + r * size + q): the expectation of the all-to-all is uploaded block by block
    blocks = [oracle.fill(count, xmpi.F32, xmpi.PAT_SIGNED, 5000 + r * size + me) for r in range(size)]  # everybody's block `me`
    for q in range(size):
        comm.fill(send.at(q * count * 4), count, xmpi.F32, xmpi.PAT_SIGNED, 5000 + me * size + q)
        comm.memcpy(want.at(q * count * 4), blocks[q].ctypes.data, count * 4)
    assert send.download(np.float32, count, byte_offset=me * count * 4).tobytes() == blocks[me].tobytes(), "device fill differs from oracle fill"
    comm.memset(recv, 0xA5, n * 4)
    comm.barrier()
    comm.alltoall(send, recv, count, xmpi.F32, xmpi.ALGO_AUTO)
    assert comm.count_mismatch(recv, want, n * 4) == 0, "alltoall 32 MiB per block"
    comm.memset(small, 0xA5, count * 4)
    comm.reduce_scatter(send, small, count, xmpi.F32, xmpi.SUM, xmpi.ALGO_AUTO)
    folded = oracle.reduce_ranks(blocks, xmpi.F32, xmpi.SUM)  # (named: the upload reads it)
    comm.memcpy(want.ptr, folded.ctypes.data, count * 4)
    assert comm.count_mismatch(small, want, count * 4) == 0, "reduce_scatter 32 MiB per block"
    for x in (send, recv, small, want):
        x.free()


SCENARIOS = {"algos": sc_algos, "sweep": sc_sweep, "memory": sc_memory, "graph": sc_graph, "parity": sc_parity, "layout": sc_layout,
             "mismatch": sc_mismatch, "fullsize": sc_fullsize, "hard": sc_hard}
