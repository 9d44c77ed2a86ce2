"""Scenarios of XMPI_F8E4M3 / XMPI_F8E5M2 (the OCP 8-bit floats, folded in f32).  Each function runs on ONE rank (a process or a thread,
tests/f8_worker.py) and checks its own results against the numpy restatement of the two types (tests/f8_ref.py): the same set of NaN
positions, every other element bit for bit.  The library never fills these buffers (its test-only fill stops at bf16): every input
comes from the host.

Inputs (rank_inputs): ranks 0 and 1 hold EVERY PAIR of encodings where the count allows (65536 elements: element i is byte i >> 8 on
rank 0 and i & 255 on rank 1 -- every two-operand tie, saturation, cancellation to +-0, subnormal sums, inf - inf and NaN) and
pseudo-random bytes otherwise; the further ranks add a small fixed set -- +0, -0, the smallest subnormal of either sign, -max, one,
and a NaN in known slots -- so that the narrowing between contributions (SUM) and its absence (SUM_WIDE) both show."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

from mpi_amd import xmpi
from tests import f8_ref as fr
from tests.scenarios import _HARD_COUNTERS, _hard_forms

AR, RD, RS = "allreduce", "reduce", "reduce_scatter"
DTYPES = fr.F8_DTYPES
OPS = (xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX, xmpi.SUM_WIDE)
BITOPS = (xmpi.BAND, xmpi.BOR, xmpi.BXOR)
# one element; around the 8-element LL line and the 16-element packet; LL lines; above ll_bytes (ragged); the 32 KiB LL limit from both
# sides; full tiles and a tail
COUNTS = (1, 7, 8, 9, 15, 16, 17, 1000, 4099, 32768, 32769, 65536 + 5)
PAIRS = 65536
NAMES = (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_DIRECT)
STEPPED = (xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_TREE, xmpi.ALGO_RING_PUSH, xmpi.ALGO_RHD_PUSH, xmpi.ALGO_TREE_PUSH)
PAD = 256  # bytes in front of and behind a device buffer that must stay as they were
SEND_PAD, RECV_PAD = 0x5E, 0xC7

ncalls = [0]


def _dtypes(args):
    """both types, or the one a test names (a job per type keeps every job at seconds on the card)"""
    return (args["dtype"],) if "dtype" in args else DTYPES


_inputs = {}
_cases = {}


def rank_inputs(dtype, count, seed, size):
    """[r] -> the bytes of rank r; computed once, never written"""
    key = (dtype, count, seed, size)
    if key not in _inputs:
        maxb = fr.LAYOUT[dtype][2]
        i = np.arange(count, dtype=np.int64)
        rng = np.random.default_rng(seed * 1000 + count)
        out = []
        for r in range(size):
            if r < 2 and count == PAIRS:
                x = ((i >> 8) if r == 0 else (i & 255)).astype(np.uint8)
            elif r < 2:
                x = rng.integers(0, 256, size=count, dtype=np.uint8)
            else:
                small = np.array([0x00, 0x80, 0x01, 0x80 | maxb, 0x01, 0x81, 0x00, 0x38 if dtype == xmpi.F8E4M3 else 0x3C], dtype=np.uint8)
                x = small[(i // 3 + r + seed) % len(small)]
                x = np.where(i % 101 == 17 + r, 0x7F, x).astype(np.uint8)
            x.setflags(write=False)
            out.append(x)
        _inputs[key] = out
    return _inputs[key]


def case(coll, dtype, count, seed, size, op):
    """([q][r] inputs, [q] expectation): allreduce / reduce: one job (q = 0); reduce-scatter: block q is a job of its own (seed + q)"""
    key = (coll, dtype, count, seed, size, op)
    if key not in _cases:
        blocks = [rank_inputs(dtype, count, seed + q, size) for q in range(size if coll == RS else 1)]
        want = [fr.reduce_ranks(b, dtype, op) for b in blocks]
        for w in want:
            w.setflags(write=False)
        _cases[key] = (blocks, want)
    return _cases[key]


def _hip_runtime():
    return ctypes.CDLL(os.environ.get("XMPI_DEVSIM_LIB") or "libamdhip64.so")


def _call(comm, coll, send, recv, count, dtype, op, algo, root, stream=None, nonblocking=False):
    if stream is not None:
        if coll == AR:
            comm.allreduce_on_stream(send, recv, count, dtype, op, stream)
        elif coll == RD:
            comm.reduce_on_stream(send, recv, count, dtype, op, root, stream)
        else:
            comm.reduce_scatter_on_stream(send, recv, count, dtype, op, stream)
        comm.stream_sync(stream)
    elif nonblocking:
        assert coll == AR
        comm.request_wait(comm.iallreduce(send, recv, count, dtype, op, algo))
    elif coll == AR:
        comm.allreduce(send, recv, count, dtype, op, algo)
    elif coll == RD:
        comm.reduce(send, recv, count, dtype, op, root, algo)
    else:
        comm.reduce_scatter(send, recv, count, dtype, op, algo)


def f8_case(comm, coll, dtype, count, op, algo=xmpi.ALGO_AUTO, root=0, inplace=False, misalign=0, mem="registered", stream=None,
            nonblocking=False, seed=300, what=""):
    """one call, checked.  mem: registered (xmpi_malloc) | host (numpy slices) | foreign (hipMalloc, never registered); misalign: the
    buffers start that many elements behind a 16-byte boundary.  Returns the result (None where it is not significant)."""
    me, size = comm.rank(), comm.size()
    blocks, wants = case(coll, dtype, count, seed, size, op)
    mine = np.concatenate([blocks[q][me] for q in range(size)]) if coll == RS else blocks[0][me]
    want = wants[me if coll == RS else 0]
    significant = coll != RD or me == root
    sb, rb, shift = mine.nbytes, count, misalign
    what = (f"{what} {coll} {xmpi.DTYPE_NAME[dtype]} count={count} op={op} algo={algo} root={root} inplace={inplace} misalign={misalign} "
            f"mem={mem} stream={stream is not None} rank {me}/{size}")
    assert not (inplace and coll == RS)
    if mem == "host":
        send = mine.copy()
        recv = send if inplace else np.zeros(rb, dtype=np.uint8)
        _call(comm, coll, send, recv, count, dtype, op, algo, root, stream, nonblocking)
        if significant:
            fr.same(recv[:count], want, dtype, what)
        if not inplace:
            assert send.tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
        ncalls[0] += 1
        return recv[:count] if significant else None
    if mem == "foreign":
        hip = _hip_runtime()
        s, r = ctypes.c_void_p(0), ctypes.c_void_p(0)
        comm.sync()
        assert hip.hipMalloc(ctypes.byref(s), ctypes.c_size_t(sb + 2 * PAD)) == 0 and hip.hipMalloc(ctypes.byref(r), ctypes.c_size_t(rb + 2 * PAD)) == 0
        sf, rf = s.value, (s.value if inplace else r.value)
    else:
        send = comm.alloc(sb + 2 * PAD)
        recv = send if inplace else comm.alloc(rb + 2 * PAD)
        sf, rf = send.ptr, recv.ptr
    simage = np.concatenate([np.full(PAD + shift, SEND_PAD, dtype=np.uint8), mine, np.full(PAD - shift, SEND_PAD, dtype=np.uint8)])
    comm.memcpy(sf, simage.ctypes.data, sb + 2 * PAD)
    if not inplace:
        comm.memset(rf, RECV_PAD, rb + 2 * PAD)
        comm.memset(rf + PAD + shift, 0xA5, rb)
    _call(comm, coll, sf + PAD + shift, rf + PAD + shift, count, dtype, op, algo, root, stream, nonblocking)
    back = np.empty((sb if inplace else rb) + 2 * PAD, dtype=np.uint8)
    comm.memcpy(back.ctypes.data, rf, back.nbytes)
    got = back[PAD + shift:PAD + shift + rb]
    pad = SEND_PAD if inplace else RECV_PAD
    assert np.all(back[:PAD + shift] == pad), f"{what}: wrote in front of the receive buffer"
    if significant:
        fr.same(got, want, dtype, what)
        assert np.all(back[PAD + shift + (sb if inplace else rb):] == pad), f"{what}: wrote past the receive buffer"
    if not inplace:
        sback = np.empty(sb + 2 * PAD, dtype=np.uint8)
        comm.memcpy(sback.ctypes.data, sf, sb + 2 * PAD)
        assert sback.tobytes() == simage.tobytes(), f"{what}: the send buffer, or bytes in front of or behind it, were written"
    if mem == "foreign":
        comm.barrier()
        assert hip.hipFree(s) == 0 and hip.hipFree(r) == 0
    else:
        send.free()
        if not inplace:
            recv.free()
    ncalls[0] += 1
    return got.copy() if significant else None


def _local_pairs(comm, dtype, nsrcs):
    """every pair of encodings (and, with more sources, the fixed small set behind them) through xmpi_reduce_local (two sources) and
    xmpi_reduce_local_n, each operator: this is what holds the card's packed conversions to the definition"""
    bufs = [comm.alloc(PAIRS) for _ in range(max(nsrcs))]
    out = comm.alloc(PAIRS)
    ins = rank_inputs(dtype, PAIRS, 300, max(nsrcs))
    for b, x in zip(bufs, ins):
        b.upload(x)
    n = 0
    for op in OPS:
        comm.memset(out, 0xA5, PAIRS)
        comm.reduce_local(out, bufs[0], bufs[1], PAIRS, dtype, op)
        fr.same(out.download(np.uint8, PAIRS), fr.reduce_ranks(ins[:2], dtype, op), dtype, f"reduce_local {xmpi.DTYPE_NAME[dtype]} op={op}")
        for ns in nsrcs:
            comm.memset(out, 0xA5, PAIRS)
            comm.reduce_local_n(out, bufs[:ns], PAIRS, dtype, op)
            fr.same(out.download(np.uint8, PAIRS), fr.reduce_ranks(ins[:ns], dtype, op), dtype, f"reduce_local_n {xmpi.DTYPE_NAME[dtype]} op={op} nsrc={ns}")
            n += 1
        n += 1
    for x in bufs + [out]:
        x.free()
    return n


def sc_pairs(comm, args):
    """exhaustive pairs: 65536 elements, every operator, both types, allreduce by AUTO and ZCOPY and xmpi_reduce_local; with 3 ranks
    or more SUM and SUM_WIDE must differ somewhere (neither can stand in for the other)"""
    me, size = comm.rank(), comm.size()
    for dtype in _dtypes(args):
        got = {}
        for op in OPS:
            for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY):
                got[op] = f8_case(comm, AR, dtype, PAIRS, op, algo, what="pairs")
        if size >= 3:
            d = fr.differing(got[xmpi.SUM], got[xmpi.SUM_WIDE], dtype)
            assert d > 0, f"SUM and SUM_WIDE of {size} ranks agree in every element ({xmpi.DTYPE_NAME[dtype]}): one aliases the other"
        else:
            assert fr.differing(got[xmpi.SUM], got[xmpi.SUM_WIDE], dtype) == 0, "two contributions: SUM_WIDE is SUM bit for bit"
        if me == 0:
            _local_pairs(comm, dtype, (2, 3))
    if me == 0:
        print(f"f8 pairs: {ncalls[0]} collective calls checked")


def _all_colls(comm, dtype, count, algo, k, **kw):
    """allreduce under every operator; allreduce in place, reduce at the first and the last rank and reduce-scatter under one operator
    each, taken in turn (k counts the calls, the same on every rank)"""
    size = comm.size()
    for op in OPS:
        f8_case(comm, AR, dtype, count, op, algo, **kw)
    f8_case(comm, AR, dtype, count, OPS[k % 5], algo, inplace=True, **kw)
    for j, root in enumerate(sorted({0, size - 1})):
        f8_case(comm, RD, dtype, count, OPS[(k + 1 + j) % 5], algo, root=root, **kw)
    f8_case(comm, RS, dtype, count, OPS[(k + 3) % 5], algo, **kw)


def sc_names(comm, args):
    """AUTO | ZCOPY | ZPUSH | LL | DIRECT at every count, both types, every collective: the same bits by every name (all are held to
    the one expectation); then buffers one element behind a 16-byte boundary"""
    me, size = comm.rank(), comm.size()
    cover = bool(args.get("cover"))
    # cover (8 processes taking turns on one card): a count of every kind -- one element, an LL line and a bit, a packet and a bit,
    # above ll_bytes and ragged, just above the LL limit --, every name at each; per (count, name) allreduce under one operator and one
    # of {allreduce in place, reduce at the last rank, reduce-scatter} under another, taken in turn: every operator, collective and
    # name meet every kind of count, not every triple
    counts = args.get("counts", [1, 9, 17, 4099, 32769] if cover else list(COUNTS))
    names = args.get("names", list(NAMES))
    ll0 = comm.get_param("dsync_ll_launches")
    k = 0
    for dtype in _dtypes(args):
        for count in counts:
            for algo in names:
                if cover:
                    f8_case(comm, AR, dtype, count, OPS[k % 5], algo)
                    op2 = OPS[(k + 2) % 5]
                    if k % 3 == 0:
                        f8_case(comm, AR, dtype, count, op2, algo, inplace=True)
                    elif k % 3 == 1:
                        f8_case(comm, RD, dtype, count, op2, algo, root=size - 1)
                    else:
                        f8_case(comm, RS, dtype, count, op2, algo)
                else:
                    _all_colls(comm, dtype, count, algo, k)
                k += 1
        for count in [c for c in (17, 4099) if c in counts]:
            for algo in (names[:2] if cover else names):
                f8_case(comm, AR, dtype, count, OPS[k % 5], algo, misalign=1)
                f8_case(comm, AR, dtype, count, OPS[(k + 2) % 5], algo, misalign=1, inplace=True)
                k += 1
    if comm.get_param("dsync") and xmpi.ALGO_LL in names:
        assert comm.get_param("dsync_ll_launches") > ll0, "the LL lines never ran"
    if me == 0:
        print(f"f8 names: {ncalls[0]} calls checked")


def sc_forms(comm, args):
    """every rank-order form of the layout, forced through its parameters (tests/scenarios.py _hard_forms) -- after every call the
    launch counters say that the form that was meant is the one that ran.  One exception, by design: a REDUCTION of these types is
    never handed to the lingering LL agent (its kernel does not know them); where the form says "by the agent" the launched LL
    kernel must have run."""
    size = comm.size()
    cover = bool(args.get("cover"))  # (8 processes on one card: one LL count and one above, the extras once)
    counts = args.get("counts", [1000, 4099] if cover else [1000, 4099, 65536 + 5])
    staged = bool(args.get("expect_staged"))
    counters = lambda: {k: comm.get_param(k) for k in _HARD_COUNTERS}
    maxb = comm.get_param("ll_max_bytes") if comm.get_param("dsync") == 1 else 0
    n = 0
    for what, algo, params, ran in _hard_forms(comm, staged):
        old = {k: comm.get_param(k) for k in params if k not in ("sync_first", "tree_reduce")}
        for k in old:
            comm.set_param(k, params[k])
        by_agent = "by the agent" in what

        def call(coll, dtype, count, op, **kw):
            if params.get("sync_first"):
                comm.sync()
            before = counters()
            f8_case(comm, coll, dtype, count, op, algo, what=what, **kw)
            after = counters()
            if by_agent:
                ll = after["dsync_ll_launches"] - before["dsync_ll_launches"]
                assert after["dsync_ll_agent"] == before["dsync_ll_agent"] and ll == (1 if count <= maxb else 0), \
                    f"{what}: an 8-bit float reduction must be launched, not handed to the agent: {before} -> {after}"
            else:
                assert ran(before, after, count), f"{what}: another form ran ({coll} {xmpi.DTYPE_NAME[dtype]} n={count} {kw}): counters {before} -> {after}"

        for dtype in _dtypes(args):
            for j, count in enumerate(counts):
                call(AR, dtype, count, xmpi.SUM_WIDE if j % 2 else xmpi.SUM)
                call(RD, dtype, count, OPS[(n + j + 2) % 5], root=size - 1)
                n += 2
                if not cover:
                    call(AR, dtype, count, OPS[(n + j) % 5])
                    n += 1
            call(AR, dtype, 4099, xmpi.SUM, misalign=1)
            n += 1
            if not cover:
                call(AR, dtype, 1000, xmpi.SUM_WIDE, inplace=True, misalign=1)
                f8_case(comm, RS, dtype, 1003, xmpi.SUM, algo, what=what)
                n += 2
        for k, v in old.items():
            comm.set_param(k, v)
    if comm.get_param("dsync") == 1:
        old = comm.get_param("ll_bytes")
        comm.set_param("ll_bytes", 0)
        for dtype in _dtypes(args):
            before = counters()
            f8_case(comm, AR, dtype, 9, xmpi.SUM, xmpi.ALGO_AUTO, what="AUTO, ll_bytes 0")
            after = counters()
            assert after["dsync_ll_launches"] == before["dsync_ll_launches"] and after["dsync_launches"] > before["dsync_launches"], (before, after)
        comm.set_param("ll_bytes", old)
    if comm.rank() == 0:
        print(f"f8 forms: {n} calls checked, each with its form confirmed by the counters")


def sc_memory(comm, args):
    """host slices, device memory nobody registered, the stream-ordered forms, non-blocking allreduces, allreduce_repeat"""
    size = comm.size()
    dsync = comm.get_param("dsync") == 1
    k = 0
    mcounts = (1000,) if args.get("cover") else (7, 1000, 20001)
    for dtype in _dtypes(args):
        for count in mcounts:
            for mem in ("host", "foreign"):
                for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY):
                    f8_case(comm, AR, dtype, count, OPS[k % 5], algo, mem=mem)
                    k += 1
                f8_case(comm, AR, dtype, count, xmpi.SUM_WIDE, xmpi.ALGO_AUTO, mem=mem, inplace=True)
                f8_case(comm, RD, dtype, count, xmpi.SUM, xmpi.ALGO_AUTO, mem=mem, root=size - 1)
                f8_case(comm, RS, dtype, count, OPS[k % 5], xmpi.ALGO_AUTO, mem=mem)
            f8_case(comm, AR, dtype, count, xmpi.SUM_WIDE, xmpi.ALGO_AUTO, nonblocking=True)
            f8_case(comm, AR, dtype, count, xmpi.SUM, xmpi.ALGO_ZPUSH, nonblocking=True, mem="host")
        st = comm.stream_create()
        for count in ((7, 20001) if args.get("cover") else (7, 1000, 20001)):
            for op in (xmpi.SUM, xmpi.SUM_WIDE, xmpi.MAX):
                f8_case(comm, AR, dtype, count, op, stream=st)
            f8_case(comm, AR, dtype, count, xmpi.SUM_WIDE, stream=st, inplace=True)
            f8_case(comm, RD, dtype, count, xmpi.PROD, stream=st, root=size - 1)
            f8_case(comm, RS, dtype, count, xmpi.MIN, stream=st)
            if dsync:  # (ranks that meet on the host: the stream-ordered forms take registered memory)
                f8_case(comm, AR, dtype, count, xmpi.SUM, stream=st, mem="foreign")
        comm.stream_destroy(st)
        # _repeat: three steps back to back, the result of the last
        count = 4099
        blocks, wants = case(AR, dtype, count, 300, size, xmpi.SUM_WIDE)
        send, recv = comm.alloc(count).upload(blocks[0][comm.rank()]), comm.alloc(count)
        for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY):
            comm.memset(recv, 0xA5, count)
            comm.allreduce_repeat(send, recv, count, dtype, xmpi.SUM_WIDE, algo, 3)
            fr.same(recv.download(np.uint8, count), wants[0], dtype, f"allreduce_repeat algo={algo}")
        send.free()
        recv.free()


def sc_graph(comm, args):
    """a captured graph of {reduce-scatter (SUM), allreduce (SUM_WIDE), reduce (MAX)}, replayed 3 times with new inputs each time"""
    me, size = comm.rank(), comm.size()
    for dtype in _dtypes(args):
        for count in (100, 9000):  # LL lines / the fold
            n = size * count
            a, b, c, d = comm.alloc(n), comm.alloc(count), comm.alloc(count), comm.alloc(count)
            st = comm.stream_create()

            def sequence():
                comm.reduce_scatter_on_stream(a, b, count, dtype, xmpi.SUM, st)
                comm.allreduce_on_stream(b, c, count, dtype, xmpi.SUM_WIDE, st)
                comm.reduce_on_stream(c, d, count, dtype, xmpi.MAX, size - 1, st)

            comm.memset(a, 0, n)
            sequence()  # (everything mapped before the capture)
            comm.stream_sync(st)
            comm.graph_begin(st)
            sequence()
            graph = comm.graph_end(st)
            for rep in range(3):
                blocks, wants = case(RS, dtype, count, 600 + 10 * rep, size, xmpi.SUM)
                a.upload(np.concatenate([blocks[q][me] for q in range(size)]))
                comm.memset(d, 0xA5, count)
                comm.barrier()  # (nobody's replay reads a buffer its owner is still filling)
                comm.graph_launch(graph, st)
                comm.stream_sync(st)
                want_c = fr.reduce_ranks(wants, dtype, xmpi.SUM_WIDE)
                fr.same(b.download(np.uint8, count), wants[me], dtype, f"graph replay {rep}: reduce_scatter count={count}")
                fr.same(c.download(np.uint8, count), want_c, dtype, f"graph replay {rep}: allreduce count={count}")
                if me == size - 1:
                    fr.same(d.download(np.uint8, count), fr.reduce_ranks([want_c] * size, dtype, xmpi.MAX), dtype, f"graph replay {rep}: reduce count={count}")
                comm.barrier()
            comm.graph_destroy(graph)
            comm.stream_destroy(st)
            for x in (a, b, c, d):
                x.free()


def _tune_class(nbytes: int) -> int:
    cls = 0
    while cls + 1 < 24 and (nbytes >> (cls + 9)) != 0:
        cls += 1
    return cls


def sc_table(comm, args):
    """a hand-written table row naming RING / RHD_PUSH / TREE, `tuned` = 1: XMPI_SUM of U8 through AUTO takes the stepped kernel
    (dsync_sched_launches), the same bytes as an 8-bit float type run the fold instead and give the defined bits"""
    size = comm.size()
    count = 20001
    counters = lambda: {k: comm.get_param(k) for k in _HARD_COUNTERS}
    tuned0 = comm.get_param("tuned")
    cls = _tune_class(count)
    for dtype in _dtypes(args):
        for coll, coll_id, algo in ((AR, xmpi.COLL_ALLREDUCE, xmpi.ALGO_RING), (AR, xmpi.COLL_ALLREDUCE, xmpi.ALGO_RHD_PUSH), (RD, xmpi.COLL_REDUCE, xmpi.ALGO_TREE)):
            comm.set_param(f"tune_algo_{coll_id}_{cls}", algo)
            comm.set_param("tuned", 1)
            before = counters()
            send, recv = comm.alloc(count), comm.alloc(count)
            comm.memset(send, 0, count)
            _call(comm, coll, send, recv, count, xmpi.U8, xmpi.SUM, xmpi.ALGO_AUTO, size - 1)
            mid = counters()
            assert mid["dsync_sched_launches"] > before["dsync_sched_launches"], f"XMPI_U8 did not take the table's schedule {algo}: {before} -> {mid}"
            for op in (xmpi.SUM, xmpi.SUM_WIDE, xmpi.MIN):
                f8_case(comm, coll, dtype, count, op, xmpi.ALGO_AUTO, root=size - 1, what=f"table row names {algo}")
            after = counters()
            assert after["dsync_sched_launches"] == mid["dsync_sched_launches"] and after["dsync_launches"] > mid["dsync_launches"], \
                f"an 8-bit float reduction through a table row naming {algo}: {mid} -> {after}"
            comm.set_param(f"tune_algo_{coll_id}_{cls}", -1)
            comm.set_param("tuned", tuned0)
            send.free()
            recv.free()


def _refusals(comm, dtype, count, forms=("blocking", "nonblocking", "repeat")):
    """every stepped name, every operator: XMPI_ERR_UNSUPPORTED; every bitwise operator by every name: XMPI_ERR_ARG"""
    size = comm.size()
    send, recv = comm.alloc(size * count), comm.alloc(count)
    comm.memset(send, 0, size * count)
    comm.memset(recv, 0x5A, count)

    def refused(code, words, coll, op, algo, form):
        try:
            if form == "repeat":
                comm.allreduce_repeat(send, recv, count, dtype, op, algo, 3)
            elif form == "stream":
                comm.allreduce_on_stream(send, recv, count, dtype, op, None)
            elif form == "local":
                comm.reduce_local(recv, send, send, count, dtype, op)
            else:
                _call(comm, coll, send, recv, count, dtype, op, algo, 0, nonblocking=form == "nonblocking")
        except xmpi.XmpiError as e:
            assert e.code == code, e
            assert all(w in str(e) for w in words), e
        else:
            raise AssertionError(f"{coll} algo={algo} op={op} on {xmpi.DTYPE_NAME[dtype]} ({form}) returned without an error")

    for algo in STEPPED:
        for op in OPS:
            for coll in (AR, RD):
                for form in forms:
                    if form != "blocking" and coll != AR:
                        continue
                    refused(xmpi.ERR_UNSUPPORTED, ("F8E4M3", "zcopy", "direct"), coll, op, algo, form)
    for op in BITOPS:
        for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_RING, xmpi.ALGO_DIRECT):
            for coll in (AR, RD, RS):
                if coll == RS and algo == xmpi.ALGO_RING:
                    continue
                refused(xmpi.ERR_ARG, ("integer type",), coll, op, algo, "blocking")
        for form in forms[1:] + ("stream", "local"):
            refused(xmpi.ERR_ARG, ("integer type",), AR, op, xmpi.ALGO_AUTO, form)
    assert np.all(recv.download(np.uint8, count) == 0x5A), "a refused call wrote into the receive buffer"
    send.free()
    recv.free()


def sc_refused(comm, args):
    """a stepped name for a reduction of these types is XMPI_ERR_UNSUPPORTED on every rank, from the arguments alone -- nothing is
    launched, announced or lent, the text names the schedules that exist -- a bitwise operator is XMPI_ERR_ARG, and the communicator
    stays usable; what has no operator runs by the stepped names as for any one-byte element (sc_moves)"""
    names = ("dsync_launches", "dsync_ll_launches", "dsync_sched_launches", "dsync_split_launches", "zc_seq", "dsync_epoch")
    for dtype in _dtypes(args):
        for count in (9, 20001):
            before = {k: comm.get_param(k) for k in names}
            _refusals(comm, dtype, count)
            assert {k: comm.get_param(k) for k in names} == before, "a refused call launched or announced something"
            f8_case(comm, AR, dtype, count, xmpi.SUM_WIDE, xmpi.ALGO_AUTO, what="after the refusals")  # the communicator is usable


def sc_mismatch(comm, args):
    """the last rank passes another 8-bit type than the others (E4M3 / E5M2 / U8), above the LL limit: different calls -- every rank
    gets XMPI_ERR_ARG at once, nothing is moved.  (Virtual devices only.)"""
    import time
    me, size = comm.rank(), comm.size()
    mine, other = args["dtypes"]
    count = 20001
    f8_case(comm, AR, mine if mine != xmpi.U8 else other, count, xmpi.SUM, xmpi.ALGO_ZCOPY)  # (everything mapped)
    a, b = comm.alloc(count), comm.alloc(count)
    comm.memset(a, 0, count)
    comm.memset(b, 0x5A, count)
    t0 = time.time()
    try:
        comm.allreduce(a, b, count, other if me == size - 1 else mine, xmpi.SUM, xmpi.ALGO_ZCOPY)
    except xmpi.XmpiError as e:
        took = time.time() - t0
        assert e.code == xmpi.ERR_ARG and "not in the same call" in str(e), e
        assert took < 5, f"the error took {took:.1f} s -- somebody waited for a clock"
        assert np.all(b.download(np.uint8, count) == 0x5A), "a peer wrote into this rank's buffer although the calls differed"
        print(f"rank {me}/{size} f8 mismatch: ok (error after {took * 1e3:.0f} ms)")
        sys.stdout.flush()
        os._exit(0)  # (the job is aborted: no finalize barrier)
    raise AssertionError("ranks in different calls returned without an error")


def sc_layout(comm, args):
    """the other layouts -- rank threads of one process, XMPI_DSYNC=0 (the host-rendezvous fold), XMPI_DSYNC=0 XMPI_ZERO_COPY=0 (the
    staged tables): the forms of the layout with their counters, host slices, then the refusals"""
    sc_forms(comm, dict(args, counts=args.get("counts", [4099])))
    for dtype in DTYPES:
        _refusals(comm, dtype, 1000, forms=("blocking",))
        f8_case(comm, AR, dtype, 1000, xmpi.SUM_WIDE, xmpi.ALGO_AUTO, mem="host")
        f8_case(comm, RS, dtype, 1000, xmpi.SUM, xmpi.ALGO_AUTO, mem="host")
        for op in OPS:
            f8_case(comm, AR, dtype, 1000, op, xmpi.ALGO_AUTO)
    if args.get("expect_staged"):
        assert comm.get_param("zc_seq") == 0 and comm.get_param("dsync_launches") == 0, "the staged tables were not what ran"
    if args.get("expect_host_fold"):
        assert comm.get_param("zc_seq") > 0 and comm.get_param("dsync_launches") == 0, "the host-rendezvous fold was not what ran"


def sc_moves(comm, args):
    """everything without an operator takes the two types as any one-byte element: bcast, allgather, all-to-all, alltoallv and Send /
    Receive / probe of all 256 encodings (NaN payloads, infinities, both zeros), bit-exact by every schedule name those accept -- the
    stepped ones included; a Receive that names the other 8-bit type is refused"""
    me, size = comm.rank(), comm.size()
    dsync = comm.get_param("dsync") == 1
    staged = bool(args.get("expect_staged"))
    n = 0
    for dtype in _dtypes(args):
        other = xmpi.F8E5M2 if dtype == xmpi.F8E4M3 else xmpi.F8E4M3
        for count in ((256,) if args.get("cover") else (256, 4099)):
            data = [np.roll(np.resize(np.arange(256, dtype=np.uint8), count), 11 * r) for r in range(size)]
            names_gather = [xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT] if staged else [xmpi.ALGO_AUTO, xmpi.ALGO_LL, xmpi.ALGO_ZCOPY, xmpi.ALGO_RING, xmpi.ALGO_DIRECT] + (
                [xmpi.ALGO_RING_PUSH] if dsync else [])
            names_bcast = [xmpi.ALGO_AUTO, xmpi.ALGO_TREE] if staged else [xmpi.ALGO_AUTO, xmpi.ALGO_LL, xmpi.ALGO_ZCOPY, xmpi.ALGO_TREE] + (
                [xmpi.ALGO_TREE_PUSH] if dsync else [])
            names_a2a = [xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT] if staged else [xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_LL, xmpi.ALGO_DIRECT]
            send, recv = comm.alloc(size * count), comm.alloc(size * count)
            for algo in names_gather:
                send.upload(data[me])
                comm.memset(recv, 0xA5, size * count)
                comm.allgather(send, recv, count, dtype, algo)
                assert recv.download(np.uint8, size * count).tobytes() == np.concatenate(data).tobytes(), f"allgather algo={algo} count={count}"
                n += 1
            for algo in names_bcast:
                root = size - 1
                if me == root:
                    recv.upload(data[root])
                else:
                    comm.memset(recv, 0xA5, count)
                comm.bcast(recv, count, dtype, root, algo)
                assert recv.download(np.uint8, count).tobytes() == data[root].tobytes(), f"bcast algo={algo} count={count}"
                n += 1
            blocks = np.concatenate([np.roll(data[me], j) for j in range(size)])  # block j is for rank j
            for algo in names_a2a:
                send.upload(blocks)
                comm.memset(recv, 0xA5, size * count)
                comm.alltoall(send, recv, count, dtype, algo)
                want = np.concatenate([np.roll(data[r], me) for r in range(size)])
                assert recv.download(np.uint8, size * count).tobytes() == want.tobytes(), f"alltoall algo={algo} count={count}"
                n += 1
            for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT) if staged else (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_DIRECT):
                send.upload(blocks)
                comm.memset(recv, 0xA5, size * count)
                sc = [count - (me + j) % 3 for j in range(size)]  # rank me sends count - (me + j) % 3 elements to rank j
                got = comm.alltoallv(send, size * count, sc, [j * count for j in range(size)], recv, size * count, [count] * size,
                                     [r * count for r in range(size)], dtype, algo)
                back = recv.download(np.uint8, size * count)
                for r in range(size):
                    k = count - (r + me) % 3
                    assert int(got[r]) == k and back[r * count:r * count + k].tobytes() == np.roll(data[r], me)[:k].tobytes(), f"alltoallv algo={algo} from {r}"
                    assert np.all(back[r * count + k:(r + 1) * count] == 0xA5), "alltoallv wrote past a block"
                n += 1
            # Send / Receive / probe round the ring of ranks: device and host buffers, blocking and stream-ordered
            nxt, prv = (me + 1) % size, (me - 1) % size
            hrecv = np.zeros(count, dtype=np.uint8)
            send.upload(data[me])
            for tag, (sbuf, rbuf) in enumerate(((send, recv), (data[me].copy(), hrecv))):
                comm.memset(recv, 0xA5, count)
                if me % 2 == 0:
                    comm.send(sbuf, count, dtype, nxt, 40 + tag)
                    assert comm.recv(rbuf, count, dtype, prv, 40 + tag) == count
                else:
                    assert comm.probe(prv, 40 + tag) == (count, dtype)
                    assert comm.recv(rbuf, count, dtype, prv, 40 + tag) == count
                    comm.send(sbuf, count, dtype, nxt, 40 + tag)
                got = recv.download(np.uint8, count) if rbuf is recv else hrecv
                assert got.tobytes() == data[prv].tobytes(), f"Send / Receive tag {40 + tag} count={count}"
                n += 1
            if dsync:
                st = comm.stream_create()
                comm.memset(recv, 0xA5, count)
                comm.sync()
                if me % 2 == 0:  # (a Send's kernel ends when its Receive has answered: somebody receives first)
                    comm.send_on_stream(send, count, dtype, nxt, 50, st)
                    comm.recv_on_stream(recv, count, dtype, prv, 50, st)
                else:
                    comm.recv_on_stream(recv, count, dtype, prv, 50, st)
                    comm.send_on_stream(send, count, dtype, nxt, 50, st)
                comm.stream_sync(st)
                assert recv.download(np.uint8, count).tobytes() == data[prv].tobytes(), "stream-ordered Send / Receive"
                comm.stream_destroy(st)
                n += 1
            send.free()
            recv.free()
        # the dtype check that exists: a message sent as one 8-bit type is not received as the other (pairs of ranks: 0 -> 1)
        if me < 2 and size >= 2:
            buf = comm.alloc(256).upload(np.arange(256, dtype=np.uint8))
            try:
                if me == 0:
                    comm.send(buf, 256, dtype, 1, 60)
                else:
                    comm.recv(buf, 256, other, 0, 60)
            except xmpi.XmpiError as e:
                assert e.code == xmpi.ERR_ARG, e
                assert me == 0 or "dtype" in str(e), e
            else:
                assert me == 0, "a Receive naming the other 8-bit type took the message"
            buf.free()
        comm.barrier()
    # xmpi_copy_local*: bytes
    if me == 0:
        x = np.arange(256, dtype=np.uint8)
        a, b, c = comm.alloc(256).upload(x), comm.alloc(256), comm.alloc(256)
        comm.copy_local(b, a, 256)
        comm.copy_local_multi([b, c], a, 256)
        assert b.download(np.uint8, 256).tobytes() == x.tobytes() and c.download(np.uint8, 256).tobytes() == x.tobytes()
        # ... and the two verification kernels take the types: identical buffers differ by nothing, NaN against NaN counts as equal
        for dtype in DTYPES:
            mx, sm, nan = comm.diff_stats(a, b, 256, dtype)
            assert mx == 0.0 and nan == 0, (mx, sm, nan)
            assert comm.diff_rel(a, b, 256, dtype) == 0.0
        # ... and read them as what they are: two DIFFERENT buffers of finite values (bytes 0x01 .. 0x70 against the same reversed,
        # both signs), the expectation from the format's own decode table -- every value, difference and sum below is exact in a
        # double, so the figures are equal, not close, and the other format's table gives other figures; then a NaN on one side only
        va = np.concatenate([np.arange(0x01, 0x71, dtype=np.uint8), np.arange(0x81, 0xF1, dtype=np.uint8)])
        vb = va[::-1].copy()
        a.upload(va)
        b.upload(vb)
        for dtype in DTYPES:
            other = xmpi.F8E5M2 if dtype == xmpi.F8E4M3 else xmpi.F8E4M3
            wa, wb = fr.widen(va, dtype).astype(np.float64), fr.widen(vb, dtype).astype(np.float64)
            want = (float(np.max(np.abs(wa - wb))), float(np.sum(np.abs(wb))), float(np.max(np.abs(wa - wb) / np.abs(wb))))
            oa, ob = fr.widen(va, other).astype(np.float64), fr.widen(vb, other).astype(np.float64)
            assert want[:2] != (float(np.max(np.abs(oa - ob))), float(np.sum(np.abs(ob))))  # (the test can tell the formats apart)
            mx, sm, nan = comm.diff_stats(a, b, len(va), dtype)
            assert (mx, sm, nan) == (want[0], want[1], 0), (xmpi.DTYPE_NAME[dtype], mx, sm, nan, want)
            assert comm.diff_rel(a, b, len(va), dtype) == want[2], (xmpi.DTYPE_NAME[dtype], want)
        b.upload(np.array([0x7F], dtype=np.uint8))
        for dtype in DTYPES:
            assert comm.diff_stats(a, b, len(va), dtype)[2] == 1 and comm.diff_rel(a, b, len(va), dtype) == float("inf")
        for t in (a, b, c):
            t.free()
        print(f"f8 moves: {n} calls checked")


def sc_kernels(comm, args):
    """single-process parity of the local kernels, one dtype per call (args["dtype"]): every pair of encodings through
    xmpi_reduce_local and xmpi_reduce_local_n with 2, 3, 8 and 16 sources, every operator; every count, aligned and one element behind
    a 16-byte boundary, through xmpi_reduce_local_n / _multi / _batch; the midpoints of the format and their neighbours as a
    three-source SUM_WIDE; kernel_mode 0 / 1 / 2 and a capped grid on a subset"""
    dtype = args["dtype"]
    name = xmpi.DTYPE_NAME[dtype]
    n = _local_pairs(comm, dtype, (2, 3, 8, 16))
    # rounding and stickiness in isolation: v + ulp/2 +- the smallest subnormal, as three sources (for E4M3 every such sum is exact in
    # f32; for E5M2 the definition is the f32 formula, which the reference computes)
    v = fr.finite_sorted(dtype)
    lo = np.arange(len(v) - 1, dtype=np.uint8)
    half = ((v[1:].astype(np.float64) - v[:-1].astype(np.float64)) / 2).astype(np.float32)
    halfb = fr.narrow(half, dtype)
    keep = fr.widen(halfb, dtype) == half  # (half an ulp is a value of the format itself from the second binade of normals on)
    assert np.count_nonzero(keep) >= len(lo) - 3 * (1 << fr.LAYOUT[dtype][0])
    lo, halfb = lo[keep], halfb[keep]
    cnt = len(lo)
    srcs = [comm.alloc(4 * cnt) for _ in range(3)]
    out = comm.alloc(4 * cnt)
    for sign in (0x00, 0x80):
        ins = [np.concatenate([lo | sign] * 4), np.concatenate([halfb | sign] * 4),
               np.concatenate([np.full(cnt, 0x00, np.uint8), np.full(cnt, 0x80, np.uint8), np.full(cnt, 0x01, np.uint8), np.full(cnt, 0x81, np.uint8)])]
        for b, x in zip(srcs, ins):
            b.upload(x)
        for op in (xmpi.SUM_WIDE, xmpi.SUM):
            comm.reduce_local_n(out, srcs, 4 * cnt, dtype, op)
            fr.same(out.download(np.uint8, 4 * cnt), fr.reduce_ranks(ins, dtype, op), dtype, f"{name}: midpoints +- the smallest subnormal, op={op}")
            n += 1
    for x in srcs + [out]:
        x.free()
    # every count, both alignments, _n / _multi (one destination aliasing a source) / _batch
    nmax = max(COUNTS)
    bufs = [comm.alloc(nmax + 32) for _ in range(9)]
    outs = [comm.alloc(nmax + 32) for _ in range(3)]
    k = 0
    for nsrc in (1, 2, 3, 8, 9):
        for count in args.get("counts", list(COUNTS)):
            ins = rank_inputs(dtype, count, 700 + nsrc, nsrc)
            for shift in (0, 1):
                op = OPS[k % 5]
                k += 1
                want = fr.reduce_ranks(ins, dtype, op)
                for b, x in zip(bufs, ins):
                    b.upload(x, byte_offset=shift)
                for o in outs:
                    comm.memset(o, 0xEE, nmax + 32)
                comm.reduce_local_n(outs[0].at(shift), [b.at(shift) for b in bufs[:nsrc]], count, dtype, op)
                alias = min(1, nsrc - 1)
                comm.reduce_local_multi([outs[1].at(shift), bufs[alias].at(shift)], [b.at(shift) for b in bufs[:nsrc]], count, dtype, op)
                for o in (outs[0], outs[1], bufs[alias]):
                    fr.same(o.download(np.uint8, count, byte_offset=shift), want, dtype, f"{name} nsrc={nsrc} count={count} shift={shift} op={op}")
                for o in outs[:2]:
                    assert np.all(o.download(np.uint8, 16, byte_offset=shift + count) == 0xEE) and np.all(o.download(np.uint8, shift) == 0xEE), "wrote outside the destination"
                n += 2
    for count in (17, 4099):  # _batch: two segments of two operands, a second destination for the first
        ins = rank_inputs(dtype, count, 800, 4)
        for b, x in zip(bufs, ins):
            b.upload(x)
        for op in OPS:
            for o in outs:
                comm.memset(o, 0xEE, nmax + 32)
            comm.reduce_local_batch([outs[0], outs[1]], [outs[2], None], [bufs[0], bufs[2]], [bufs[1], bufs[3]], [count, count], dtype, op)
            w0, w1 = fr.reduce_ranks(ins[:2], dtype, op), fr.reduce_ranks(ins[2:], dtype, op)
            fr.same(outs[0].download(np.uint8, count), w0, dtype, f"{name} batch op={op}")
            fr.same(outs[2].download(np.uint8, count), w0, dtype, f"{name} batch, second destination op={op}")
            fr.same(outs[1].download(np.uint8, count), w1, dtype, f"{name} batch, segment 1 op={op}")
            n += 1
    for mode, cap in ((0, 0), (1, 0), (2, 0), (-1, 3)):
        comm.set_param("kernel_mode", mode)
        comm.set_param("grid_cap", cap)
        for nsrc in (2, 8, 9):
            ins = rank_inputs(dtype, 65536 + 5, 700 + nsrc, nsrc)
            for b, x in zip(bufs, ins):
                b.upload(x)
            for op in (xmpi.SUM, xmpi.SUM_WIDE):
                comm.reduce_local_n(outs[0], bufs[:nsrc], 65536 + 5, dtype, op)
                fr.same(outs[0].download(np.uint8, 65536 + 5), fr.reduce_ranks(ins, dtype, op), dtype, f"{name} kernel_mode={mode} grid_cap={cap} nsrc={nsrc} op={op}")
                n += 1
    comm.set_param("kernel_mode", -1)
    comm.set_param("grid_cap", 0)
    for x in bufs + outs:
        x.free()
    print(f"f8 kernels {name}: {n} launches checked")


SCENARIOS = {"pairs": sc_pairs, "names": sc_names, "forms": sc_forms, "memory": sc_memory, "graph": sc_graph, "table": sc_table, "refused": sc_refused,
             "mismatch": sc_mismatch, "layout": sc_layout, "moves": sc_moves, "kernels": sc_kernels}
