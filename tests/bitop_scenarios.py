"""Scenarios of XMPI_BAND / XMPI_BOR / XMPI_BXOR (bitwise reductions of U8 / I32 / I64).  Each function runs on ONE rank (a process or
a thread, tests/bitop_worker.py) and compares its own results BIT FOR BIT with the numpy restatement (tests/bitop_ref.py): the
operators are exact, associative and commutative, so every schedule -- the stepped and the push forms included -- has the one
expectation.  XOR is what shows a contribution applied twice (x ^ x = 0) where a MAX hides it and a sum merely doubles."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

from mpi_amd import xmpi
from tests import bitop_ref as br
from tests.scenarios import _HARD_COUNTERS, _hard_forms

AR, RD, RS = "allreduce", "reduce", "reduce_scatter"
DTYPES, OPS = br.DTYPES, br.OPS
COUNTS = (1, 7, 8, 9, 1000, 4099, 65536 + 5)  # one element, around one packet, the agent's 8 KiB and the LL lines' 32 KiB either side, ragged tails
NAMES = {AR: (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_DIRECT, xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_RING_PUSH,
               xmpi.ALGO_RHD_PUSH),
         RD: (xmpi.ALGO_TREE, xmpi.ALGO_TREE_PUSH, xmpi.ALGO_DIRECT, xmpi.ALGO_ZCOPY, xmpi.ALGO_AUTO),
         RS: (xmpi.ALGO_ZCOPY, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_DIRECT, xmpi.ALGO_AUTO)}
PAD = 256  # bytes in front of and behind a device buffer that must stay as they were
SEND_PAD, RECV_PAD = 0x5E, 0xC7
LAUNCH_COUNTERS = ("dsync_launches", "dsync_ll_launches", "dsync_sched_launches", "dsync_split_launches", "zc_seq", "dsync_epoch")

ncalls = [0]  # checked calls of this rank
_cases = {}  # (coll, dtype, op, count, seed, size) -> ([q][r] inputs, [q] expectation): computed once, never written


def case(coll, dtype, op, count, seed, size):
    """allreduce / reduce: one job (q = 0); reduce-scatter: block q of every rank's send buffer is a job of its own (seed + 100 q)"""
    key = (coll, dtype, op, count, seed, size)
    if key not in _cases:
        blocks = [br.rank_inputs(dtype, count, seed + 100 * q, size, op) for q in range(size if coll == RS else 1)]
        want = [br.reduce_ranks(b, op) for b in blocks]
        for x in [a for b in blocks for a in b] + want:
            x.setflags(write=False)
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
        assert coll != RS
        comm.request_wait(comm.iallreduce(send, recv, count, dtype, op, algo) if coll == AR else comm.ireduce(send, recv, count, dtype, op, root, algo))
    elif coll == AR:
        comm.allreduce(send, recv, count, dtype, op, algo)
    elif coll == RD:
        comm.reduce(send, recv, count, dtype, op, root, algo)
    else:
        comm.reduce_scatter(send, recv, count, dtype, op, algo)


def same_bits(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} elements differ, first at {bad[0]}: got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


def bit_case(comm, coll, dtype, op, count, algo=xmpi.ALGO_AUTO, root=0, inplace=False, misalign=0, mem="registered", stream=None, nonblocking=False,
             seed=4000, what=""):
    """one call, checked.  mem: registered (xmpi_malloc) | host (numpy slices) | foreign (hipMalloc, never registered); misalign: the
    buffers start that many elements behind a 16-byte boundary (the one-element-per-lane paths).  Returns the result (None where it is
    not significant: a reduce on a rank that is not the root)."""
    me, size = comm.rank(), comm.size()
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    blocks, wants = case(coll, dtype, op, count, seed, size)
    mine = np.concatenate([blocks[q][me] for q in range(size)]) if coll == RS else blocks[0][me]
    want = wants[me if coll == RS else 0]
    significant = coll != RD or me == root
    sb, rb, shift = mine.nbytes, count * es, misalign * es
    what = (f"{what} {coll} {xmpi.DTYPE_NAME[dtype]} {br.OP_NAME[op]} count={count} algo={algo} root={root} inplace={inplace} misalign={misalign} "
            f"mem={mem} stream={stream is not None} nonblocking={nonblocking} rank {me}/{size}")
    assert not (inplace and coll == RS)
    if mem == "host":
        send = mine.copy()
        recv = send if inplace else np.full(rb // es, 0, dtype=npdt)
        _call(comm, coll, send, recv, count, dtype, op, algo, root, stream, nonblocking)
        if significant:
            same_bits(recv[:count], want, what)
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
    got = back[PAD + shift:PAD + shift + rb].copy().view(npdt)
    pad = SEND_PAD if inplace else RECV_PAD
    assert np.all(back[:PAD + shift] == pad), f"{what}: wrote in front of the receive buffer"
    if significant:
        same_bits(got, want, what)
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
    return got if significant else None


def _dtypes(args):
    return [args["dtype"]] if "dtype" in args else list(DTYPES)


def _name_shapes(size):
    """(collective, name, keywords) of every call shape of the names scenario: 33 of them"""
    shapes = []
    for algo in NAMES[AR]:
        shapes += [(AR, algo, {}), (AR, algo, {"inplace": True})]
    for algo in NAMES[RD]:
        shapes += [(RD, algo, {"root": root}) for root in sorted({0, size - 1})]
    shapes += [(RS, algo, {}) for algo in NAMES[RS]]
    return shapes


def sc_names(comm, args):
    """every algorithm name the collective accepts x three operators x {1, 7, 8, 9, 1000, 4099, 65536 + 5} elements x {allreduce out of
    and in place, reduce at the first and the last rank, reduce-scatter}, for the dtypes of args["dtype"] (all three without): the same
    bits by every name -- each is held to the one expectation.
    args["cover"]: a covering subset instead of the product, for a job whose calls are slow (8 processes that share ONE GPU take turns
    on it: a collective costs tens of milliseconds there).  Every one of the 33 call shapes runs at three counts -- one of {1, 7, 8, 9},
    1000, one of {4099, 65536 + 5}: around one packet, LL lines, above them -- with the count of each class and the operator
    rotating, so that every shape meets all three operators and every size class, every count is met, and every allreduce and
    reduce name meets both large counts.  The product itself runs on the virtual devices at this size and on the GPU
    with 2 and 3 processes."""
    me, size = comm.rank(), comm.size()
    counts = args.get("counts", list(COUNTS))
    ll0, sched0 = comm.get_param("dsync_ll_launches"), comm.get_param("dsync_sched_launches")
    if args.get("cover"):
        dtypes = _dtypes(args)
        for i, (coll, algo, kw) in enumerate(_name_shapes(size)):
            for j, cls in enumerate(((1, 7, 8, 9), (1000,), (4099, 65536 + 5))):
                # (i + i // 2: the two shapes of a name -- out of and in place, first and last root -- get different counts, and not
                # always the same way round)
                bit_case(comm, coll, dtypes[(i + j) % len(dtypes)], OPS[(i + j) % 3], cls[(i + i // 2) % len(cls)], algo, **kw)
    else:
        for dtype in _dtypes(args):
            for op in OPS:
                for count in counts:
                    for coll, algo, kw in _name_shapes(size):
                        bit_case(comm, coll, dtype, op, count, algo, **kw)
    if comm.get_param("dsync") == 1:
        assert comm.get_param("dsync_ll_launches") > ll0, "the LL lines never ran"
        assert comm.get_param("dsync_sched_launches") > sched0, "the stepped kernels never ran"
    if me == 0:
        print(f"bitop names: {ncalls[0]} calls checked")


def _ops(args, rot):
    """the three operators -- or, args["cover"] (a job whose calls are slow: sc_names), one of them, the next one each time"""
    return (OPS[rot[0] % 3],) if args.get("cover") else OPS


def _forms(comm, staged):
    """tests/scenarios.py _hard_forms (one kernel at unroll 1 and 2, meet / body / done and its system-scope body, LL launched and by
    the agent, ZPUSH, DIRECT; the host rendezvous; the staged tables) with the collectives each takes, and the stepped kernels in
    their pull and push forms: (what, algo, parameters, counters afterwards, collectives)"""
    forms = [(what, algo, params, ran, (AR, RD, RS)) for what, algo, params, ran in _hard_forms(comm, staged)]
    if staged:
        stepped = lambda b, a, unit: a["zc_seq"] == 0 and a["dsync_launches"] == 0
    elif comm.get_param("dsync") != 1:  # the host-driven step tables: no rendezvous of the zero-copy fold, no device meeting
        stepped = lambda b, a, unit: a["zc_seq"] == b["zc_seq"] and a["dsync_launches"] == 0
    else:  # one stepped kernel per rank
        stepped = lambda b, a, unit: a["dsync_sched_launches"] == b["dsync_sched_launches"] + 1 and a["dsync_ll_launches"] == b["dsync_ll_launches"]
    for what, algo, colls in (("RING, pull", xmpi.ALGO_RING, (AR,)), ("RING, push", xmpi.ALGO_RING_PUSH, (AR,)), ("RHD, pull", xmpi.ALGO_RHD, (AR,)),
                              ("RHD, push", xmpi.ALGO_RHD_PUSH, (AR,)), ("TREE, pull", xmpi.ALGO_TREE, (RD,)), ("TREE, push", xmpi.ALGO_TREE_PUSH, (RD,))):
        forms.append((what, algo, {}, stepped, colls))
    return forms


def sc_forms(comm, args):
    """every form of the layout, forced through its parameters; after every call the launch counters say that the form that was
    meant is the one that ran; per form, buffers one element behind a 16-byte boundary (the one-element-per-lane paths).
    args["cover"]: one operator per form and dtype, rotating, instead of all three (see sc_names).  The reduce-scatter call of each
    form runs under the form's settings and is checked by its bits only: the counters' rules are written for allreduce and reduce"""
    size = comm.size()
    big, mid = args.get("counts", [65536 + 5, 4099])  # (every rank has a chunk: the counters are exact)
    staged = bool(args.get("expect_staged"))
    counters = lambda: {k: comm.get_param(k) for k in _HARD_COUNTERS}
    # (a job of one dtype starts the rotation at that dtype: the three jobs of a size together give every form all three operators)
    n, nrs, rot = 0, 0, [_dtypes(args)[0]]
    for what, algo, params, ran, colls in _forms(comm, staged):
        old = {k: comm.get_param(k) for k in params if k not in ("sync_first", "tree_reduce")}
        for k in old:
            comm.set_param(k, params[k])

        def call(coll, dtype, op, count, **kw):
            if coll not in colls:
                return 0
            if params.get("sync_first"):
                comm.sync()
            before = counters()
            bit_case(comm, coll, dtype, op, count, algo, what=what, **kw)
            after = counters()
            assert coll == RS or ran(before, after, count * xmpi.DTYPE_SIZE[dtype]), \
                f"{what}: another form ran ({coll} {xmpi.DTYPE_NAME[dtype]} n={count} {kw}): counters {before} -> {after}"
            return 1

        for dtype in _dtypes(args):
            for op in _ops(args, rot):
                n += call(AR, dtype, op, big) + call(AR, dtype, op, mid) + call(RD, dtype, op, mid, root=size - 1) + call(RD, dtype, op, 1000, root=0)
                n += call(AR, dtype, op, mid, misalign=1) + call(AR, dtype, op, 1000, inplace=True, misalign=1) + call(RD, dtype, op, mid, root=size - 1, misalign=1)
                nrs += call(RS, dtype, op, 1003)  # (U8: no block but the first is 16-byte aligned; checked by its bits, not by the counters)
            rot[0] += 1
        for k, v in old.items():
            comm.set_param(k, v)
    if comm.rank() == 0:
        print(f"bitop forms: {n} calls checked, each with its form confirmed by the counters; {nrs} reduce-scatter calls under the same settings checked by their bits")


def sc_memory(comm, args):
    """host slices, device memory nobody registered, the stream-ordered forms, xmpi_iallreduce / xmpi_ireduce (args["cover"]: the
    non-blocking and stream-ordered calls with one rotating operator instead of all three, see sc_names)"""
    size = comm.size()
    dsync = comm.get_param("dsync") == 1
    k, rot = 0, [1]
    for dtype in DTYPES:
        st = comm.stream_create()
        for count in (7, 1000, 20001):
            op = OPS[k % 3]  # (every operator meets every dtype and every count)
            k += 1
            rot[0] += 1
            for mem in ("host", "foreign"):
                for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY):
                    bit_case(comm, AR, dtype, op, count, algo, mem=mem)
                bit_case(comm, AR, dtype, op, count, xmpi.ALGO_AUTO, mem=mem, inplace=True)
                bit_case(comm, RD, dtype, op, count, xmpi.ALGO_AUTO, mem=mem, root=size - 1)
                bit_case(comm, RS, dtype, op, count, xmpi.ALGO_AUTO, mem=mem)
            for o in _ops(args, rot):
                bit_case(comm, AR, dtype, o, count, xmpi.ALGO_AUTO, nonblocking=True)
                bit_case(comm, RD, dtype, o, count, xmpi.ALGO_AUTO, nonblocking=True, root=size - 1)
                bit_case(comm, AR, dtype, o, count, stream=st)
                bit_case(comm, RD, dtype, o, count, stream=st, root=size - 1)
                bit_case(comm, RS, dtype, o, count, stream=st)
            bit_case(comm, AR, dtype, op, count, xmpi.ALGO_ZPUSH, nonblocking=True, mem="host")
            bit_case(comm, RD, dtype, op, count, xmpi.ALGO_TREE, nonblocking=True, mem="host", root=0)
            bit_case(comm, AR, dtype, op, count, stream=st, inplace=True)
            if dsync:  # (ranks that meet on the host: the stream-ordered forms take registered memory)
                bit_case(comm, AR, dtype, op, count, stream=st, mem="foreign")
        comm.stream_destroy(st)
    if comm.rank() == 0:
        print(f"bitop memory: {ncalls[0]} calls checked")


def sc_graph(comm, args):
    """a captured graph of {reduce-scatter, allreduce}, one operator each, replayed 3 times with new inputs each time"""
    me, size = comm.rank(), comm.size()
    k = 0
    for dtype in DTYPES:
        es = xmpi.DTYPE_SIZE[dtype]
        npdt = xmpi.NUMPY_DTYPE[dtype]
        for count in (100, 9000):  # LL lines / the fold
            op_rs, op_ar = OPS[k % 3], OPS[(k + 1) % 3]
            k += 1
            a, b, c = comm.alloc(size * count * es), comm.alloc(count * es), comm.alloc(count * es)
            st = comm.stream_create()

            def sequence():
                comm.reduce_scatter_on_stream(a, b, count, dtype, op_rs, st)
                comm.allreduce_on_stream(b, c, count, dtype, op_ar, st)

            sequence()  # (everything mapped before the capture)
            comm.stream_sync(st)
            comm.graph_begin(st)
            sequence()
            graph = comm.graph_end(st)
            for rep in range(3):
                blocks, want_b = case(RS, dtype, op_rs, count, 4600 + 1000 * rep, size)
                a.upload(np.concatenate([blocks[q][me] for q in range(size)]))
                comm.memset(c, 0xA5, count * es)
                comm.barrier()  # (nobody's replay reads a buffer its owner is still filling)
                comm.graph_launch(graph, st)
                comm.stream_sync(st)
                same_bits(b.download(npdt, count), want_b[me], f"graph replay {rep}: reduce_scatter {br.OP_NAME[op_rs]} count={count}")
                same_bits(c.download(npdt, count), br.reduce_ranks(want_b, op_ar), f"graph replay {rep}: allreduce {br.OP_NAME[op_ar]} count={count}")
                comm.barrier()
            comm.graph_destroy(graph)
            comm.stream_destroy(st)
            for x in (a, b, c):
                x.free()


def _refused(fn, what, text="integer type"):
    try:
        fn()
    except xmpi.XmpiError as e:
        assert e.code == xmpi.ERR_ARG, f"{what}: {e}"
        assert text is None or text in str(e), f"{what}: the error does not say why: {e}"
    else:
        raise AssertionError(f"{what}: returned without an error")


def _entries(comm, send, recv, count, dtype, op, st, with_local=True):
    """(name, call) for every entry that takes an operator"""
    size = comm.size()
    e = [("allreduce", lambda: comm.allreduce(send, recv, count, dtype, op, xmpi.ALGO_AUTO)),
         ("allreduce RING", lambda: comm.allreduce(send, recv, count, dtype, op, xmpi.ALGO_RING)),
         ("reduce", lambda: comm.reduce(send, recv, count, dtype, op, size - 1, xmpi.ALGO_AUTO)),
         ("reduce_scatter", lambda: comm.reduce_scatter(send, recv, count, dtype, op, xmpi.ALGO_AUTO)),
         ("iallreduce", lambda: comm.request_wait(comm.iallreduce(send, recv, count, dtype, op, xmpi.ALGO_AUTO))),
         ("ireduce", lambda: comm.request_wait(comm.ireduce(send, recv, count, dtype, op, 0, xmpi.ALGO_AUTO))),
         ("allreduce_on_stream", lambda: comm.allreduce_on_stream(send, recv, count, dtype, op, st)),
         ("reduce_on_stream", lambda: comm.reduce_on_stream(send, recv, count, dtype, op, 0, st)),
         ("reduce_scatter_on_stream", lambda: comm.reduce_scatter_on_stream(send, recv, count, dtype, op, st)),
         ("allreduce_repeat", lambda: comm.allreduce_repeat(send, recv, count, dtype, op, xmpi.ALGO_AUTO, 3)),
         ("allreduce_repeat ZCOPY", lambda: comm.allreduce_repeat(send, recv, count, dtype, op, xmpi.ALGO_ZCOPY, 3))]
    if with_local:
        es = xmpi.DTYPE_SIZE[dtype]
        a, b = send.at(0), send.at(count * es)
        e += [("reduce_local", lambda: comm.reduce_local(recv, a, b, count, dtype, op)),
              ("reduce_local_n", lambda: comm.reduce_local_n(recv, [a, b], count, dtype, op)),
              ("reduce_local_multi", lambda: comm.reduce_local_multi([recv], [a, b], count, dtype, op)),
              ("reduce_local_batch", lambda: comm.reduce_local_batch([recv], None, [a], [b], [count], dtype, op))]
    return e


def _captured(comm, dtype, st):
    """the same refusal while a stream is being captured: nothing is recorded for the refused calls (the counters do not move), the
    capture goes on, and the graph holds the one valid call that followed"""
    me, size = comm.rank(), comm.size()
    count = 9000
    blocks, want = case(AR, xmpi.I32, xmpi.BXOR, count, 4700, size)
    send, recv, fsend, frecv = comm.alloc(count * 4).upload(blocks[0][me]), comm.alloc(count * 4), comm.alloc(size * count * 8), comm.alloc(count * 8)
    comm.allreduce_on_stream(send, recv, count, xmpi.I32, xmpi.BXOR, st)  # (everything mapped before the capture)
    comm.stream_sync(st)
    comm.memset(recv, 0xA5, count * 4)
    comm.barrier()
    comm.graph_begin(st)
    before = {k: comm.get_param(k) for k in LAUNCH_COUNTERS}
    for op in OPS:
        what = f"captured, {br.OP_NAME[op]} on {xmpi.DTYPE_NAME[dtype]}"
        _refused(lambda: comm.allreduce_on_stream(fsend, frecv, count, dtype, op, st), f"{what}: allreduce")
        _refused(lambda: comm.reduce_on_stream(fsend, frecv, count, dtype, op, 0, st), f"{what}: reduce")
        _refused(lambda: comm.reduce_scatter_on_stream(fsend, frecv, count, dtype, op, st), f"{what}: reduce_scatter")
    assert {k: comm.get_param(k) for k in LAUNCH_COUNTERS} == before, f"a refused call recorded or announced something while capturing ({xmpi.DTYPE_NAME[dtype]})"
    comm.allreduce_on_stream(send, recv, count, xmpi.I32, xmpi.BXOR, st)
    graph = comm.graph_end(st)
    comm.graph_launch(graph, st)
    comm.stream_sync(st)
    same_bits(recv.download(np.int32, count), want[0], f"the captured allreduce behind the refusals ({xmpi.DTYPE_NAME[dtype]})")
    comm.barrier()
    comm.graph_destroy(graph)
    for x in (send, recv, fsend, frecv):
        x.free()


def sc_float_refused(comm, args):
    """each bitwise operator with each of the four float types at every entry that takes an operator: XMPI_ERR_ARG on every rank, from
    the arguments alone -- the launch counters do not move, the receive buffer keeps its bytes, xmpi_last_error says that a bitwise
    operator needs an integer type -- and a following XMPI_SUM call succeeds"""
    me, size = comm.rank(), comm.size()
    st = comm.stream_create()
    n = 0
    for dtype in br.FLOAT_DTYPES:
        es = xmpi.DTYPE_SIZE[dtype]
        for count in (9, 20001):
            send, recv = comm.alloc(size * count * es), comm.alloc(count * es)
            comm.memset(send, 0, size * count * es)
            comm.memset(recv, 0x5A, count * es)
            for op in OPS:
                before = {k: comm.get_param(k) for k in LAUNCH_COUNTERS}
                for name, fn in _entries(comm, send, recv, count, dtype, op, st):
                    _refused(fn, f"{name} {br.OP_NAME[op]} on {xmpi.DTYPE_NAME[dtype]} count={count}")
                    n += 1
                assert {k: comm.get_param(k) for k in LAUNCH_COUNTERS} == before, f"a refused call launched or announced something ({br.OP_NAME[op]}, {xmpi.DTYPE_NAME[dtype]})"
            assert np.all(recv.download(np.uint8, count * es) == 0x5A), "a refused call wrote into the receive buffer"
            # the communicator is usable: XMPI_SUM of the same type (zeros), then a bitwise call on an integer type
            comm.allreduce(send, recv, count, dtype, xmpi.SUM, xmpi.ALGO_AUTO)
            assert np.all(recv.download(np.uint8, count * es) == 0), "XMPI_SUM after the refusals"
            send.free()
            recv.free()
            bit_case(comm, AR, xmpi.I32, xmpi.BXOR, count, what="after the refusals")
        if comm.get_param("dsync") == 1:
            _captured(comm, dtype, st)
    comm.stream_destroy(st)
    if me == 0:
        print(f"bitop float types: {n} calls refused")


def sc_bad_op(comm, args):
    """operators 8 and -1: XMPI_ERR_ARG at every entry, nothing launched, the communicator usable"""
    size = comm.size()
    st = comm.stream_create()
    count = 1000
    send, recv = comm.alloc(size * count * 4), comm.alloc(count * 4)
    comm.memset(send, 0, size * count * 4)
    comm.memset(recv, 0x5A, count * 4)
    before = {k: comm.get_param(k) for k in LAUNCH_COUNTERS}
    for op in (8, -1):
        for dtype in (xmpi.I32, xmpi.F32):
            # (xmpi_allreduce_repeat hands an operator it does not know to the collective underneath: its refusal is the same one)
            for name, fn in _entries(comm, send, recv, count, dtype, op, st):
                _refused(fn, f"{name} op={op} on {xmpi.DTYPE_NAME[dtype]}", None)
    assert {k: comm.get_param(k) for k in LAUNCH_COUNTERS} == before, "a refused call launched or announced something"
    assert np.all(recv.download(np.uint8, count * 4) == 0x5A), "a refused call wrote into the receive buffer"
    assert xmpi.BXOR == 7, "the last operator"
    send.free()
    recv.free()
    comm.stream_destroy(st)
    bit_case(comm, AR, xmpi.I32, xmpi.BXOR, count, what="after the refusals")


def sc_mismatch(comm, args):
    """XMPI_BOR on rank 0 against XMPI_BXOR on the others, above the LL limit: different calls -- every rank gets XMPI_ERR_ARG at once,
    nothing is moved.  (Virtual devices only.)"""
    import time
    me = comm.rank()
    dtype = args.get("dtype", xmpi.I32)
    es = xmpi.DTYPE_SIZE[dtype]
    count = 20001
    bit_case(comm, AR, dtype, xmpi.BOR, count, xmpi.ALGO_ZCOPY)  # (everything mapped)
    a, b = comm.alloc(count * es), comm.alloc(count * es)
    comm.memset(a, 0x33, count * es)
    comm.memset(b, 0x5A, count * es)
    t0 = time.time()
    try:
        comm.allreduce(a, b, count, dtype, xmpi.BOR if me == 0 else xmpi.BXOR, xmpi.ALGO_ZCOPY)
    except xmpi.XmpiError as e:
        took = time.time() - t0
        assert e.code == xmpi.ERR_ARG and "not in the same call" in str(e), e
        assert took < 5, f"the error took {took:.1f} s -- somebody waited for a clock"
        assert np.all(b.download(np.uint8, count * es) == 0x5A), "a peer wrote into this rank's buffer although the calls differed"
        print(f"rank {me}/{comm.size()} bitop mismatch: ok (error after {took * 1e3:.0f} ms)")
        sys.stdout.flush()
        os._exit(0)  # (the job is aborted: no finalize barrier)
    raise AssertionError("ranks in different calls returned without an error")


def sc_layout(comm, args):
    """the other layouts -- rank threads of one process, XMPI_DSYNC=0 (the host-rendezvous fold and the host-driven step tables),
    XMPI_DSYNC=0 XMPI_ZERO_COPY=0 (the staged tables: reduce2 and its batch): the forms of the layout with their counters (sc_forms),
    host slices, and a float type refused"""
    sc_forms(comm, dict(args, counts=args.get("counts", [4099, 1000])))
    size = comm.size()
    k = 0
    for dtype in DTYPES:
        op = OPS[k % 3]
        k += 1
        bit_case(comm, AR, dtype, op, 1000, xmpi.ALGO_AUTO, mem="host")
        bit_case(comm, RD, dtype, op, 1000, xmpi.ALGO_TREE, mem="host", root=size - 1)
        bit_case(comm, RS, dtype, op, 1000, xmpi.ALGO_AUTO, mem="host")
    send, recv = comm.alloc(size * 4000), comm.alloc(4000)
    for op in OPS:
        _refused(lambda: comm.allreduce(send, recv, 1000, xmpi.F32, op, xmpi.ALGO_AUTO), f"allreduce {br.OP_NAME[op]} on f32")
        _refused(lambda: comm.reduce_scatter(send, recv, 1000, xmpi.F32, op, xmpi.ALGO_AUTO), f"reduce_scatter {br.OP_NAME[op]} on f32")
    send.free()
    recv.free()
    if args.get("expect_staged"):
        assert comm.get_param("zc_seq") == 0 and comm.get_param("dsync_launches") == 0, "the staged tables were not what ran"
    if args.get("expect_host_fold"):
        assert comm.get_param("zc_seq") > 0 and comm.get_param("dsync_launches") == 0, "the host-rendezvous fold was not what ran"


def _local_check(comm, written, own, bufs, ins, want, nsrc, count, shift, dtype, what, aliased=()):
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    for o in written:
        same_bits(o.download(npdt, count, byte_offset=shift * es), want, what)
    for o in own:
        assert np.all(o.download(np.uint8, 16, byte_offset=(shift + count) * es) == 0xEE), f"{what}: the kernel wrote past the end"
        assert np.all(o.download(np.uint8, shift * es) == 0xEE), f"{what}: the kernel wrote in front of the destination"
    for j, b in enumerate(bufs[:nsrc]):
        if j not in aliased:
            assert b.download(npdt, count, byte_offset=shift * es).tobytes() == ins[j].tobytes(), f"{what}: a source was modified"


def _local_inputs(dtype, op, count, nsrc, seed=4050):
    key = ("local", dtype, op, count, nsrc, seed)
    if key not in _cases:
        ins = br.rank_inputs(dtype, count, seed, max(nsrc, 2), op)[:nsrc]
        _cases[key] = (ins, br.reduce_ranks(ins, op))
    return _cases[key]


def _local_case(comm, dtype, op, nsrc, ndst, count, shift, bufs, outs, what):
    """xmpi_reduce_local_multi (ndst destinations, the last one aliasing a source) or, ndst == 0, xmpi_reduce_local_n into one
    destination of its own: every destination holds the result, nothing is written past it, no other source is touched"""
    es = xmpi.DTYPE_SIZE[dtype]
    ins, want = _local_inputs(dtype, op, count, nsrc)
    for b, x in zip(bufs, ins):
        b.upload(x, byte_offset=shift * es)
    alias = min(1, nsrc - 1)
    own = outs[:max(1, ndst) - (1 if ndst else 0)]
    for o in own:
        comm.memset(o, 0xEE, (count + 2) * es + 16)
    if ndst:
        written = own + [bufs[alias]]
        comm.reduce_local_multi([o.at(shift * es) for o in written], [b.at(shift * es) for b in bufs[:nsrc]], count, dtype, op)
    else:
        written = own
        comm.reduce_local_n(own[0].at(shift * es), [b.at(shift * es) for b in bufs[:nsrc]], count, dtype, op)
    _local_check(comm, written, own, bufs, ins, want, nsrc, count, shift, dtype, what, aliased=(alias,) if ndst else ())


def _local_two(comm, dtype, op, count, shift, bufs, outs, what):
    """xmpi_reduce_local (two operands) and xmpi_reduce_local_batch (three segments of different lengths, a second destination for
    the first, in one call)"""
    es = xmpi.DTYPE_SIZE[dtype]
    npdt = xmpi.NUMPY_DTYPE[dtype]
    ins, want = _local_inputs(dtype, op, count, 2, 4060)
    for b, x in zip(bufs, ins):
        b.upload(x, byte_offset=shift * es)
    for o in outs[:4]:
        comm.memset(o, 0xEE, (count + 2) * es + 16)
    comm.reduce_local(outs[0].at(shift * es), bufs[0].at(shift * es), bufs[1].at(shift * es), count, dtype, op)
    _local_check(comm, outs[:1], outs[:1], bufs, ins, want, 2, count, shift, dtype, what + " reduce_local")
    cuts = [0, count // 3, count // 2, count]  # (segment starts at odd element offsets: their alignment differs)
    seg = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(3)]
    at = lambda buf, i: buf.at((shift + seg[i][0]) * es)
    comm.reduce_local_batch([at(outs[1], i) for i in range(3)], [at(outs[2], 0), None, None], [at(bufs[0], i) for i in range(3)], [at(bufs[1], i) for i in range(3)],
                            [n for _, n in seg], dtype, op)
    _local_check(comm, outs[1:2], outs[1:2], bufs, ins, want, 2, count, shift, dtype, what + " reduce_local_batch")
    n0 = seg[0][1]
    same_bits(outs[2].download(npdt, n0, byte_offset=shift * es), want[:n0], what + " reduce_local_batch, second destination")
    assert np.all(outs[2].download(np.uint8, 16, byte_offset=(shift + n0) * es) == 0xEE), f"{what}: the second destination was written past its segment"


def sc_local(comm, args):
    """single-process kernel parity of xmpi_reduce_local, _local_n, _local_multi and _local_batch, one dtype per call (args["dtype"]),
    three operators: 1..9 and 16 sources (the run-time-count kernels: the bitwise operators are not source-unrolled), 1 / 2 / 8
    destinations with one aliasing a source, every count, aligned and one element behind a 16-byte boundary, and every count and
    both alignments under kernel_mode 0 / 1 / 2; then a capped grid (more than one tile per block)"""
    dtype = args["dtype"]
    es = xmpi.DTYPE_SIZE[dtype]
    nmax = max(COUNTS)
    bufs = [comm.alloc((nmax + 2) * es) for _ in range(16)]
    outs = [comm.alloc((nmax + 2) * es + 16) for _ in range(7)]
    counts = args.get("counts", list(COUNTS))
    n = 0
    for op in OPS:
        name = f"{xmpi.DTYPE_NAME[dtype]} {br.OP_NAME[op]}"
        for nsrc in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
            for count in counts:
                for shift in (0, 1):
                    for ndst in (0, 1, 2, 8):
                        if nsrc in (1, 2, 8, 16) or ndst in (0, 8) or count >= 4099:  # (3..7 and 9 sources take the same kernel as 16: thinned)
                            _local_case(comm, dtype, op, nsrc, ndst, count, shift, bufs, outs, f"{name} nsrc={nsrc} ndst={ndst} count={count} shift={shift}")
                            n += 1
        for mode in (0, 1, 2):
            comm.set_param("kernel_mode", mode)
            for count in counts:
                for shift in (0, 1):
                    _local_two(comm, dtype, op, count, shift, bufs, outs, f"{name} kernel_mode={mode} count={count} shift={shift}")
                    for nsrc, ndst in ((2, 0), (3, 1), (8, 8), (9, 2)):
                        _local_case(comm, dtype, op, nsrc, ndst, count, shift, bufs, outs, f"{name} kernel_mode={mode} nsrc={nsrc} ndst={ndst} count={count} shift={shift}")
                    n += 6
        comm.set_param("kernel_mode", -1)
        comm.set_param("grid_cap", 3)
        for count in (4099, 65536 + 5):
            _local_two(comm, dtype, op, count, 0, bufs, outs, f"{name} grid_cap=3 count={count}")
            for nsrc, ndst in ((2, 0), (8, 8), (9, 1)):
                _local_case(comm, dtype, op, nsrc, ndst, count, 0, bufs, outs, f"{name} grid_cap=3 nsrc={nsrc} ndst={ndst} count={count}")
            n += 5
        comm.set_param("grid_cap", 0)
    for x in bufs + outs:
        x.free()
    print(f"bitop local kernels {xmpi.DTYPE_NAME[dtype]}: {n} launches checked")


SCENARIOS = {"names": sc_names, "forms": sc_forms, "memory": sc_memory, "graph": sc_graph, "float_refused": sc_float_refused, "bad_op": sc_bad_op,
             "mismatch": sc_mismatch, "layout": sc_layout, "local": sc_local}
