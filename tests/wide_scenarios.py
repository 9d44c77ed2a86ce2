"""Scenarios of XMPI_SUM_WIDE (f16 / bf16 accumulated in f32 in rank order, rounded once).  Each function runs on ONE rank (a process
or a thread, tests/wide_worker.py) and checks its own results against the numpy restatement of the operator (tests/wide_ref.py)
under hard_inputs.same_floats(..., op=SUM): the same set of NaN positions, every other element bit for bit.  Inputs are
tests/hard_inputs.py's -- `special` (NaNs, infinities, signed zeros, subnormals planted so that every ordered pair meets) and `dense`
(full mantissas) -- so order and special values show."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

from mpi_amd import xmpi
from tests import hard_inputs as hi
from tests import wide_ref as wr
from tests.scenarios import _HARD_COUNTERS, _hard_forms

AR, RD, RS = "allreduce", "reduce", "reduce_scatter"
DTYPES = wr.WIDE_DTYPES
COUNTS = (1, 7, 8, 9, 1000, 4099, 65536 + 5)  # one element, around one packet, LL lines, above ll_bytes (ragged), full tiles + a tail
NAMES = (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_DIRECT)
STEPPED = (xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_TREE, xmpi.ALGO_RING_PUSH, xmpi.ALGO_RHD_PUSH, xmpi.ALGO_TREE_PUSH)
PAD = 256  # bytes in front of and behind a device buffer that must stay as they were
SEND_PAD, RECV_PAD = 0x5E, 0xC7

ncalls = [0]  # checked calls of this rank
_cases = {}  # (coll, dtype, count, seed, size, kind) -> ([q][r] inputs, [q] wide expectation, [q] XMPI_SUM expectation): computed once, never written


def case(coll, dtype, count, seed, size, kind):
    """allreduce / reduce: one job (q = 0); reduce-scatter: block q of every rank's send buffer is a job of its own (seed + 100 q)"""
    key = (coll, dtype, count, seed, size, kind)
    if key not in _cases:
        blocks = [hi.rank_inputs(dtype, count, seed + 100 * q, size, xmpi.SUM, kind) for q in range(size if coll == RS else 1)]
        wide = [wr.wide_sum(b, dtype) for b in blocks]
        narrow = [hi.np_reduce_ranks(b, dtype, xmpi.SUM) for b in blocks]
        for x in [a for b in blocks for a in b] + wide + narrow:
            x.setflags(write=False)
        _cases[key] = (blocks, wide, narrow)
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


def wide_case(comm, coll, dtype, count, algo=xmpi.ALGO_AUTO, kind="special", root=0, inplace=False, misalign=0, mem="registered", stream=None,
              nonblocking=False, op=xmpi.SUM_WIDE, seed=9000, what=""):
    """one call, checked.  mem: registered (xmpi_malloc) | host (numpy slices) | foreign (hipMalloc, never registered); misalign: the
    buffers start that many elements behind a 16-byte boundary (the one-element-per-lane paths); op: SUM_WIDE, or SUM -- the same
    inputs through the operator that rounds after every rank, held to ITS expectation.  Returns the result (None where it is not
    significant: a reduce on a rank that is not the root)."""
    me, size = comm.rank(), comm.size()
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    blocks, wide, narrow = case(coll, dtype, count, seed, size, kind)
    mine = np.concatenate([blocks[q][me] for q in range(size)]) if coll == RS else blocks[0][me]
    want = (wide if op == xmpi.SUM_WIDE else narrow)[me if coll == RS else 0]
    significant = coll != RD or me == root
    sb, rb, shift = mine.nbytes, count * es, misalign * es
    what = (f"{what} {coll} {xmpi.DTYPE_NAME[dtype]} count={count} algo={algo} op={op} {kind} root={root} inplace={inplace} misalign={misalign} "
            f"mem={mem} stream={stream is not None} rank {me}/{size}")
    assert not (inplace and coll == RS)
    if mem == "host":
        send = mine.copy()
        recv = send if inplace else np.full(rb // es, 0, dtype=npdt)
        _call(comm, coll, send, recv, count, dtype, op, algo, root, stream, nonblocking)
        if significant:
            hi.same_floats(recv[:count], want, dtype, xmpi.SUM, what)
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
    simage = np.concatenate([np.full(PAD + shift, SEND_PAD, dtype=np.uint8), mine.view(np.uint8), np.full(PAD - shift, SEND_PAD, dtype=np.uint8)])
    comm.memcpy(sf, simage.ctypes.data, sb + 2 * PAD)
    if not inplace:
        comm.memset(rf, RECV_PAD, rb + 2 * PAD)
        comm.memset(rf + PAD + shift, 0xA5, rb)
    _call(comm, coll, sf + PAD + shift, rf + PAD + shift, count, dtype, op, algo, root, stream, nonblocking)
    back = np.empty((sb if inplace else rb) + 2 * PAD, dtype=np.uint8)
    comm.memcpy(back.ctypes.data, rf, back.nbytes)
    got = back[PAD + shift:PAD + shift + rb].view(npdt)
    pad = SEND_PAD if inplace else RECV_PAD
    assert np.all(back[:PAD + shift] == pad), f"{what}: wrote in front of the receive buffer"
    if significant:
        hi.same_floats(got, want, dtype, xmpi.SUM, what)
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


def _all_colls(comm, dtype, count, algo, kind, **kw):
    """allreduce out of and in place, reduce at the first and the last rank, reduce-scatter"""
    size = comm.size()
    wide_case(comm, AR, dtype, count, algo, kind, **kw)
    wide_case(comm, AR, dtype, count, algo, kind, inplace=True, **kw)
    for root in sorted({0, size - 1}):
        wide_case(comm, RD, dtype, count, algo, kind, root=root, **kw)
    wide_case(comm, RS, dtype, count, algo, kind, **kw)


def sc_names(comm, args):
    """AUTO | ZCOPY | ZPUSH | LL | DIRECT at every count, both types, every collective: the same bits by every name (all are held to
    the one expectation); `special` inputs, and `dense` ones at the counts either side of ll_bytes.  With 3 ranks or more the result
    differs from XMPI_SUM's of the same inputs -- from the library's, not only from numpy's."""
    me, size = comm.rank(), comm.size()
    counts = args.get("counts", list(COUNTS))
    names = args.get("names", list(NAMES))
    ll0 = comm.get_param("dsync_ll_launches")
    for dtype in DTYPES:
        for count in counts:
            for algo in names:
                _all_colls(comm, dtype, count, algo, "special")
        for count in [c for c in (1000, 4099) if c in counts]:
            for algo in names:
                _all_colls(comm, dtype, count, algo, "dense", seed=9500)
        if size >= 3 and 4099 in counts:
            got_wide = wide_case(comm, AR, dtype, 4099, xmpi.ALGO_ZCOPY, "dense", seed=9500)
            got_sum = wide_case(comm, AR, dtype, 4099, xmpi.ALGO_ZCOPY, "dense", seed=9500, op=xmpi.SUM)
            d = wr.differing(got_wide, got_sum, dtype)
            assert d >= 4099 // 10, f"SUM_WIDE and SUM differ in {d} of 4099 dense {xmpi.DTYPE_NAME[dtype]} elements only: one aliases the other"
    if comm.get_param("dsync") and xmpi.ALGO_LL in names:
        assert comm.get_param("dsync_ll_launches") > ll0, "the LL lines never ran"
    if me == 0:
        print(f"wide names: {ncalls[0]} calls checked")


def sc_forms(comm, args):
    """every rank-order form of the layout, forced through its parameters (tests/scenarios.py _hard_forms: one kernel with unroll 1
    and 2, meet / body / done, its system-scope body, LL launched and by the agent, ZPUSH, DIRECT; the host rendezvous; the staged
    tables) -- after every call the launch counters say that the form that was meant is the one that ran; plus, per form, buffers one
    element behind a 16-byte boundary (the one-element-per-lane paths) and AUTO with ll_bytes = 0 (the fold at an LL size)"""
    size = comm.size()
    counts = args.get("counts", [1000, 4099, 65536 + 5])  # (every rank has a chunk: the counters are exact)
    staged = bool(args.get("expect_staged"))
    counters = lambda: {k: comm.get_param(k) for k in _HARD_COUNTERS}
    n = 0
    for what, algo, params, ran in _hard_forms(comm, staged):
        old = {k: comm.get_param(k) for k in params if k not in ("sync_first", "tree_reduce")}
        for k in old:
            comm.set_param(k, params[k])

        def call(coll, dtype, count, **kw):
            if params.get("sync_first"):
                comm.sync()
            before = counters()
            wide_case(comm, coll, dtype, count, algo, what=what, **kw)
            after = counters()
            assert ran(before, after, count * xmpi.DTYPE_SIZE[dtype]), \
                f"{what}: another form ran ({coll} {xmpi.DTYPE_NAME[dtype]} n={count} {kw}): counters {before} -> {after}"

        for dtype in DTYPES:
            for count in counts:
                call(AR, dtype, count)
                call(RD, dtype, count, root=size - 1)  # (staged AUTO: short enough for the TREE table of plan.cpp -- DIRECT runs instead)
                n += 2
            call(AR, dtype, 4099, misalign=1)
            call(AR, dtype, 1000, inplace=True, misalign=1, kind="dense")
            wide_case(comm, RS, dtype, 1003, algo, what=what)  # (blocks of 2006 bytes: no block but the first is 16-byte aligned)
            n += 3
        for k, v in old.items():
            comm.set_param(k, v)
    if comm.get_param("dsync") == 1:
        old = comm.get_param("ll_bytes")
        comm.set_param("ll_bytes", 0)
        for dtype in DTYPES:
            before = counters()
            wide_case(comm, AR, dtype, 9, xmpi.ALGO_AUTO, what="AUTO, ll_bytes 0")
            after = counters()
            assert after["dsync_ll_launches"] == before["dsync_ll_launches"] and after["dsync_launches"] > before["dsync_launches"], (before, after)
        comm.set_param("ll_bytes", old)
    if comm.rank() == 0:
        print(f"wide forms: {n} calls checked, each with its form confirmed by the counters")


def sc_memory(comm, args):
    """host slices, device memory nobody registered, the stream-ordered forms, a non-blocking allreduce"""
    size = comm.size()
    dsync = comm.get_param("dsync") == 1
    for dtype in DTYPES:
        for count in (7, 1000, 20001):
            for mem in ("host", "foreign"):
                for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY):
                    wide_case(comm, AR, dtype, count, algo, mem=mem)
                wide_case(comm, AR, dtype, count, xmpi.ALGO_AUTO, mem=mem, inplace=True)
                wide_case(comm, RD, dtype, count, xmpi.ALGO_AUTO, mem=mem, root=size - 1)
                wide_case(comm, RS, dtype, count, xmpi.ALGO_AUTO, mem=mem)
            wide_case(comm, AR, dtype, count, xmpi.ALGO_AUTO, nonblocking=True)
            wide_case(comm, AR, dtype, count, xmpi.ALGO_ZPUSH, nonblocking=True, mem="host")
        st = comm.stream_create()
        for count in (7, 1000, 20001):
            wide_case(comm, AR, dtype, count, stream=st)
            wide_case(comm, AR, dtype, count, stream=st, inplace=True, kind="dense")
            wide_case(comm, RD, dtype, count, stream=st, root=size - 1)
            wide_case(comm, RS, dtype, count, stream=st)
            if dsync:  # (ranks that meet on the host: the stream-ordered forms take registered memory)
                wide_case(comm, AR, dtype, count, stream=st, mem="foreign")
        comm.stream_destroy(st)


def sc_graph(comm, args):
    """a captured graph of {reduce-scatter, allreduce, reduce} with XMPI_SUM_WIDE, replayed 3 times with new inputs each time"""
    me, size = comm.rank(), comm.size()
    for dtype in DTYPES:
        es = xmpi.DTYPE_SIZE[dtype]
        npdt = xmpi.NUMPY_DTYPE[dtype]
        for count in (100, 9000):  # LL lines / the fold
            n = size * count
            a, b, c, d = comm.alloc(n * es), comm.alloc(count * es), comm.alloc(count * es), comm.alloc(count * es)
            st = comm.stream_create()

            def sequence():
                comm.reduce_scatter_on_stream(a, b, count, dtype, xmpi.SUM_WIDE, st)
                comm.allreduce_on_stream(b, c, count, dtype, xmpi.SUM_WIDE, st)
                comm.reduce_on_stream(c, d, count, dtype, xmpi.SUM_WIDE, size - 1, st)

            sequence()  # (everything mapped before the capture)
            comm.stream_sync(st)
            comm.graph_begin(st)
            sequence()
            graph = comm.graph_end(st)
            for rep in range(3):
                blocks, wide, _ = case(RS, dtype, count, 9600 + 1000 * rep, size, "special" if rep != 1 else "dense")
                a.upload(np.concatenate([blocks[q][me] for q in range(size)]))
                comm.memset(d, 0xA5, count * es)
                comm.barrier()  # (nobody's replay reads a buffer its owner is still filling)
                comm.graph_launch(graph, st)
                comm.stream_sync(st)
                want_c = wr.wide_sum(wide, dtype)
                hi.same_floats(b.download(npdt, count), wide[me], dtype, xmpi.SUM, f"graph replay {rep}: reduce_scatter count={count}")
                hi.same_floats(c.download(npdt, count), want_c, dtype, xmpi.SUM, f"graph replay {rep}: allreduce count={count}")
                if me == size - 1:
                    hi.same_floats(d.download(npdt, count), wr.wide_sum([want_c] * size, dtype), dtype, xmpi.SUM, f"graph replay {rep}: reduce count={count}")
                comm.barrier()
            comm.graph_destroy(graph)
            comm.stream_destroy(st)
            for x in (a, b, c, d):
                x.free()


def sc_other_types(comm, args):
    """XMPI_SUM_WIDE on f32 and i32 IS XMPI_SUM: the same bits by every name -- and the same CALL: a job in which some ranks pass
    SUM_WIDE and the others SUM on f32, above the LL limit (where the kernels compare their call signatures), completes"""
    me, size = comm.rank(), comm.size()
    for dtype in (xmpi.F32, xmpi.I32):
        for count in (9, 1000, 20001):
            if dtype == xmpi.F32:
                ins = hi.rank_inputs(dtype, count, 9700, size, xmpi.SUM, "special")
            else:
                ins = [hi.bits_of(x, xmpi.F32).view(np.int32) for x in hi.rank_inputs(xmpi.F32, count, 9700, size, xmpi.SUM, "dense")]
            want = ins[0].copy()
            with np.errstate(all="ignore"):
                for x in ins[1:]:
                    want = want + x  # (numpy: wrapping int32 additions, IEEE f32 additions -- left to right)
            send, recv = comm.alloc(count * 4).upload(ins[me]), comm.alloc(count * 4)
            for algo in NAMES:
                for op in (xmpi.SUM_WIDE, xmpi.SUM, xmpi.SUM_WIDE if me % 2 else xmpi.SUM):
                    comm.memset(recv, 0xA5, count * 4)
                    comm.allreduce(send, recv, count, dtype, op, algo)
                    got = recv.download(xmpi.NUMPY_DTYPE[dtype], count)
                    if dtype == xmpi.F32:
                        hi.same_floats(got, want, dtype, xmpi.SUM, f"f32 count={count} algo={algo} op={op}")
                    else:
                        assert got.tobytes() == want.tobytes(), f"i32 count={count} algo={algo} op={op}"
            send.free()
            recv.free()
    # two operands: xmpi_reduce_local maps the operator (the same bits, tests/test_wide_cpu.py)
    for dtype in DTYPES:
        ins = hi.rank_inputs(dtype, 4099, 9800, 2, xmpi.SUM, "special")
        a, b, out = comm.alloc(4099 * 2).upload(ins[0]), comm.alloc(4099 * 2).upload(ins[1]), comm.alloc(4099 * 2)
        comm.reduce_local(out, a, b, 4099, dtype, xmpi.SUM_WIDE)
        hi.same_floats(out.download(xmpi.NUMPY_DTYPE[dtype], 4099), wr.wide_sum(ins, dtype), dtype, xmpi.SUM, "reduce_local")
        for x in (a, b, out):
            x.free()


def _tune_class(nbytes: int) -> int:
    cls = 0
    while cls + 1 < 24 and (nbytes >> (cls + 9)) != 0:
        cls += 1
    return cls


def sc_table(comm, args):
    """a hand-written table row naming RING, `tuned` = 1: XMPI_SUM through AUTO takes the ring kernel (dsync_sched_launches), XMPI_SUM_WIDE
    through AUTO runs the fold instead and gives the wide bits; the same for a row naming TREE for reduce"""
    size = comm.size()
    count = 20001
    counters = lambda: {k: comm.get_param(k) for k in _HARD_COUNTERS}
    tuned0 = comm.get_param("tuned")
    for dtype in DTYPES:
        cls = _tune_class(count * xmpi.DTYPE_SIZE[dtype])
        for coll, coll_id, algo in ((AR, xmpi.COLL_ALLREDUCE, xmpi.ALGO_RING), (AR, xmpi.COLL_ALLREDUCE, xmpi.ALGO_RHD_PUSH), (RD, xmpi.COLL_REDUCE, xmpi.ALGO_TREE)):
            comm.set_param(f"tune_algo_{coll_id}_{cls}", algo)
            comm.set_param("tuned", 1)
            before = counters()
            # (the ring and the tree associate in orders of their own: this call shows WHICH kernel ran, not its bits)
            send, recv = comm.alloc(count * 2), comm.alloc(count * 2)
            comm.memset(send, 0, count * 2)
            _call(comm, coll, send, recv, count, dtype, xmpi.SUM, xmpi.ALGO_AUTO, size - 1)
            mid = counters()
            assert mid["dsync_sched_launches"] > before["dsync_sched_launches"], f"XMPI_SUM did not take the table's schedule {algo}: {before} -> {mid}"
            wide_case(comm, coll, dtype, count, xmpi.ALGO_AUTO, root=size - 1, what=f"table row names {algo}")
            wide_case(comm, coll, dtype, count, xmpi.ALGO_AUTO, root=size - 1, kind="dense", what=f"table row names {algo}")
            after = counters()
            assert after["dsync_sched_launches"] == mid["dsync_sched_launches"] and after["dsync_launches"] > mid["dsync_launches"], \
                f"XMPI_SUM_WIDE through a table row naming {algo}: {mid} -> {after}"
            comm.set_param(f"tune_algo_{coll_id}_{cls}", -1)
            comm.set_param("tuned", tuned0)
            send.free()
            recv.free()


def sc_refused(comm, args):
    """every stepped name with XMPI_SUM_WIDE on f16 / bf16: XMPI_ERR_UNSUPPORTED on every rank, from the arguments alone -- nothing is
    launched, announced or lent, the text names the schedules that exist -- and the communicator stays usable; on f32 the same
    names run (the operator is XMPI_SUM there)"""
    me, size = comm.rank(), comm.size()
    names = ("dsync_launches", "dsync_ll_launches", "dsync_sched_launches", "dsync_split_launches", "zc_seq", "dsync_epoch")
    for dtype in DTYPES:
        for count in (9, 20001):
            send, recv = comm.alloc(size * count * 2), comm.alloc(count * 2)
            comm.memset(send, 0, size * count * 2)
            comm.memset(recv, 0x5A, count * 2)
            for algo in STEPPED:
                for coll in (AR, RD):
                    before = {k: comm.get_param(k) for k in names}
                    for form in ("blocking", "nonblocking", "repeat"):
                        if form != "blocking" and coll != AR:
                            continue
                        try:
                            if form == "repeat":
                                comm.allreduce_repeat(send, recv, count, dtype, xmpi.SUM_WIDE, algo, 3)
                            else:
                                _call(comm, coll, send, recv, count, dtype, xmpi.SUM_WIDE, algo, 0, nonblocking=form == "nonblocking")
                        except xmpi.XmpiError as e:
                            assert e.code == xmpi.ERR_UNSUPPORTED, e
                            assert "SUM_WIDE" in str(e) and "zcopy" in str(e) and "direct" in str(e), e
                        else:
                            raise AssertionError(f"{coll} algo={algo} with XMPI_SUM_WIDE on {xmpi.DTYPE_NAME[dtype]} ({form}) returned without an error")
                    assert {k: comm.get_param(k) for k in names} == before, f"a refused call launched or announced something (algo {algo})"
            assert np.all(recv.download(np.uint8, count * 2) == 0x5A), "a refused call wrote into the receive buffer"
            send.free()
            recv.free()
            wide_case(comm, AR, dtype, count, xmpi.ALGO_AUTO, what="after the refusals")  # the communicator is usable
    # f32: SUM_WIDE is SUM, so a stepped name is a schedule like any other
    count = 4099
    ins = hi.rank_inputs(xmpi.F32, count, 9900, size, xmpi.SUM, "dense")
    send, a, b = comm.alloc(count * 4).upload(ins[me]), comm.alloc(count * 4), comm.alloc(count * 4)
    comm.allreduce(send, a, count, xmpi.F32, xmpi.SUM, xmpi.ALGO_RING)
    comm.allreduce(send, b, count, xmpi.F32, xmpi.SUM_WIDE, xmpi.ALGO_RING)
    assert a.download(np.uint8, count * 4).tobytes() == b.download(np.uint8, count * 4).tobytes(), "f32 RING: SUM_WIDE is not SUM"
    for x in (send, a, b):
        x.free()


def sc_mismatch(comm, args):
    """XMPI_SUM on the last rank against XMPI_SUM_WIDE on the others, f16 / bf16, above the LL limit: different calls -- every rank gets
    XMPI_ERR_ARG at once, nothing is moved.  (Virtual devices only.)"""
    import time
    me, size = comm.rank(), comm.size()
    dtype = xmpi.BF16 if args.get("bf16") else xmpi.F16
    count = 20001
    wide_case(comm, AR, dtype, count, xmpi.ALGO_ZCOPY)  # (everything mapped)
    a, b = comm.alloc(count * 2), comm.alloc(count * 2)
    comm.memset(a, 0, count * 2)
    comm.memset(b, 0x5A, count * 2)
    t0 = time.time()
    try:
        comm.allreduce(a, b, count, dtype, xmpi.SUM if me == size - 1 else xmpi.SUM_WIDE, xmpi.ALGO_ZCOPY)
    except xmpi.XmpiError as e:
        took = time.time() - t0
        assert e.code == xmpi.ERR_ARG and "not in the same call" in str(e), e
        assert took < 5, f"the error took {took:.1f} s -- somebody waited for a clock"
        assert np.all(b.download(np.uint8, count * 2) == 0x5A), "a peer wrote into this rank's buffer although the calls differed"
        print(f"rank {me}/{size} wide mismatch: ok (error after {took * 1e3:.0f} ms)")
        sys.stdout.flush()
        os._exit(0)  # (the job is aborted: no finalize barrier)
    raise AssertionError("ranks in different calls returned without an error")


def sc_layout(comm, args):
    """the other layouts -- rank threads of one process, XMPI_DSYNC=0 (the host-rendezvous fold), XMPI_DSYNC=0 XMPI_ZERO_COPY=0 (the
    staged tables: allreduce, a reduce short enough that staged AUTO picks the TREE table for XMPI_SUM, reduce-scatter): the forms of
    the layout with their counters (sc_forms), then the refusals"""
    sc_forms(comm, dict(args, counts=args.get("counts", [1000, 4099])))
    size = comm.size()
    for dtype in DTYPES:
        send, recv = comm.alloc(1000 * 2), comm.alloc(1000 * 2)
        comm.memset(send, 0, 2000)
        for algo, coll in ((xmpi.ALGO_RING, AR), (xmpi.ALGO_RHD, AR), (xmpi.ALGO_TREE, RD)):
            try:
                _call(comm, coll, send, recv, 1000, dtype, xmpi.SUM_WIDE, algo, size - 1)
            except xmpi.XmpiError as e:
                assert e.code == xmpi.ERR_UNSUPPORTED and "SUM_WIDE" in str(e), e
            else:
                raise AssertionError(f"{coll} algo={algo} with XMPI_SUM_WIDE returned without an error")
        send.free()
        recv.free()
        wide_case(comm, AR, dtype, 1000, xmpi.ALGO_AUTO, mem="host")
        wide_case(comm, RS, dtype, 1000, xmpi.ALGO_AUTO, mem="host", kind="dense")
    if args.get("expect_staged"):
        assert comm.get_param("zc_seq") == 0 and comm.get_param("dsync_launches") == 0, "the staged tables were not what ran"
    if args.get("expect_host_fold"):
        assert comm.get_param("zc_seq") > 0 and comm.get_param("dsync_launches") == 0, "the host-rendezvous fold was not what ran"


def _local_case(comm, dtype, nsrc, ndst, count, shift, kind, bufs, outs, what):
    """xmpi_reduce_local_multi (ndst destinations, the last one aliasing a source) or, ndst == 0, xmpi_reduce_local_n into one
    destination of its own: every destination holds the wide sum, nothing is written past it, no other source is touched"""
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    ins = hi.rank_inputs(dtype, count, 9050, nsrc, xmpi.SUM, kind)
    want = wr.wide_sum(ins, dtype)
    for b, x in zip(bufs, ins):
        b.upload(x, byte_offset=shift * es)
    alias = min(1, nsrc - 1)
    own = outs[:max(1, ndst) - (1 if ndst else 0)]
    for o in own:
        comm.memset(o, 0xEE, (count + 2) * es + 16)
    if ndst:
        written = own + [bufs[alias]]
        comm.reduce_local_multi([o.at(shift * es) for o in written], [b.at(shift * es) for b in bufs[:nsrc]], count, dtype, xmpi.SUM_WIDE)
    else:
        written = own
        comm.reduce_local_n(own[0].at(shift * es), [b.at(shift * es) for b in bufs[:nsrc]], count, dtype, xmpi.SUM_WIDE)
    for o in written:
        hi.same_floats(o.download(npdt, count, byte_offset=shift * es), want, dtype, xmpi.SUM, what)
    for o in own:
        assert np.all(o.download(np.uint8, 16, byte_offset=(shift + count) * es) == 0xEE), f"{what}: the kernel wrote past the end"
        assert np.all(o.download(np.uint8, shift * es) == 0xEE), f"{what}: the kernel wrote in front of the destination"
    for j, b in enumerate(bufs[:nsrc]):
        if not (ndst and j == alias):
            assert b.download(npdt, count, byte_offset=shift * es).tobytes() == ins[j].tobytes(), f"{what}: a source was modified"


def sc_kernels(comm, args):
    """single-process kernel parity of xmpi_reduce_local_n and xmpi_reduce_local_multi with XMPI_SUM_WIDE, one dtype per call
    (args["dtype"]): 1..9 and 16 sources (every unrolled count and the run-time-count kernel), 1 / 2 / 8 destinations with one
    aliasing a source, every count, aligned and one element behind a 16-byte boundary; then kernel_mode 0 / 1 / 2 and a capped grid
    (more than one tile per block) on a subset.  This is where the real hardware's f32 subnormal handling and its f32 -> f16
    conversion are held to numpy."""
    dtype = args["dtype"]
    es = xmpi.DTYPE_SIZE[dtype]
    nmax = max(COUNTS)
    bufs = [comm.alloc((nmax + 2) * es) for _ in range(16)]
    outs = [comm.alloc((nmax + 2) * es + 16) for _ in range(7)]
    n = 0
    for nsrc in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        for count in args.get("counts", list(COUNTS)):
            for shift in (0, 1):
                for ndst in (0, 1, 2, 8):
                    kind = "dense" if (count == 4099 and ndst == 2) else "special"
                    _local_case(comm, dtype, nsrc, ndst, count, shift, kind, bufs, outs, f"{xmpi.DTYPE_NAME[dtype]} nsrc={nsrc} ndst={ndst} count={count} shift={shift} {kind}")
                    n += 1
    for mode, cap in ((0, 0), (1, 0), (2, 0), (-1, 3)):
        comm.set_param("kernel_mode", mode)
        comm.set_param("grid_cap", cap)
        for nsrc in (2, 8, 9):
            for count in (4099, 65536 + 5):
                for ndst in (0, 1, 8):
                    _local_case(comm, dtype, nsrc, ndst, count, 0, "special", bufs, outs, f"{xmpi.DTYPE_NAME[dtype]} kernel_mode={mode} grid_cap={cap} nsrc={nsrc} ndst={ndst} count={count}")
                    n += 1
    comm.set_param("kernel_mode", -1)
    comm.set_param("grid_cap", 0)
    # three sources or more: not the bits of XMPI_SUM (the library's own, on the same buffers)
    ins = hi.rank_inputs(dtype, 4099, 9050, 8, xmpi.SUM, "dense")
    for b, x in zip(bufs, ins):
        b.upload(x)
    comm.reduce_local_n(outs[0], bufs[:8], 4099, dtype, xmpi.SUM_WIDE)
    comm.reduce_local_n(outs[1], bufs[:8], 4099, dtype, xmpi.SUM)
    d = wr.differing(outs[0].download(xmpi.NUMPY_DTYPE[dtype], 4099), outs[1].download(xmpi.NUMPY_DTYPE[dtype], 4099), dtype)
    assert d >= 4099 // 10, f"SUM_WIDE and SUM differ in {d} of 4099 dense elements only"
    for x in bufs + outs:
        x.free()
    print(f"wide kernels {xmpi.DTYPE_NAME[dtype]}: {n} launches checked")


SCENARIOS = {"kernels": sc_kernels, "names": sc_names, "forms": sc_forms, "memory": sc_memory, "graph": sc_graph, "other_types": sc_other_types, "table": sc_table,
             "refused": sc_refused, "mismatch": sc_mismatch, "layout": sc_layout}
