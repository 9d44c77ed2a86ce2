"""Scenarios of xmpi_alltoallv: an all-to-all with a count per pair, the counts read on the device and exchanged by the kernels.
Each function runs on ONE rank (a process or a thread, tests/vcoll_worker.py) and checks its own results.  The expectation is a
numpy re-slicing of the ranks' inputs; a copy is exact, so there is no tolerance anywhere: the receive buffer is compared WHOLE
(the gaps between the blocks and a 64-byte guard behind it included, pre-filled with 0xA5), the send buffer is compared unchanged,
and the received counts are compared."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from mpi_amd import xmpi

GUARD = 64
FILL = 0xA5
COUNTS = (0, 1, 3, 17, 1000, 4099, 70001)
DTYPES = (xmpi.U8, xmpi.F16, xmpi.I64)
LAYOUTS = ("packed", "slotted", "oddbase", "elem", "skewed")  # (oddbase, elem: U8 only)
ALGOS = (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_DIRECT)

_data = {}


def rank_bytes(rank: int, nbytes: int) -> np.ndarray:
    """rank `rank`'s send buffer of nbytes: computed once, shared by the cases, never written"""
    key = (rank, nbytes)
    if key not in _data:
        a = np.random.default_rng(7700 + rank).integers(0, 256, size=nbytes, dtype=np.uint8)
        a.setflags(write=False)
        _data[key] = a
    return _data[key]


def count(frm: int, to: int, seed: int, size: int, kind: str = "packed") -> int:
    """a fixed function of (from, to, seed): one rank's whole row is zero and another rank's whole column is zero"""
    if kind == "skewed":  # one block 64 x the others
        return 64 * 1000 if (frm, to) == (seed % size, (seed + 2) % size) else 1000
    if kind == "equal":
        return seed
    if frm == seed % size or to == (seed + 1) % size:
        return 0
    return COUNTS[(frm * 5 + to * 3 + seed) % len(COUNTS)]  # (5 and 3 are coprime to len(COUNTS): sender and receiver both count)


def plan(rank: int, size: int, seed: int, kind: str) -> dict:
    """the arrays rank `rank` passes, in elements"""
    sc = [count(rank, j, seed, size, kind) for j in range(size)]
    rc = [count(r, rank, seed, size, kind) for r in range(size)]
    if kind in ("packed", "skewed", "equal"):
        caps = list(rc)
        sd = [sum(sc[:j]) for j in range(size)]
        rd = [sum(caps[:r]) for r in range(size)]
    elif kind == "slotted":  # gaps between the blocks on both sides, capacity = count + 5
        caps = [n + 5 for n in rc]
        sd = [sum(sc[:j]) + 2 * j + 1 for j in range(size)]
        rd = [sum(caps[:r]) + 3 * r for r in range(size)]
    else:
        # U8: every block at a multiple of 16 plus a residue -- oddbase: 3 on both sides (congruent, not aligned: head, packets,
        # tail); elem: 1 against 6 (not congruent: one element per lane)
        caps = list(rc)
        rs, rr = (3, 3) if kind == "oddbase" else (1, 6)
        sd, rd, at = [], [], 0
        for j in range(size):
            sd.append(at + rs)
            at += (sc[j] + rs + 15) // 16 * 16
        at = 0
        for r in range(size):
            rd.append(at + rr)
            at += (caps[r] + rr + 15) // 16 * 16
    se = max([d + n for d, n in zip(sd, sc)] + [0]) + (4 if kind == "slotted" else 0)
    re_ = max([d + n for d, n in zip(rd, caps)] + [0]) + (4 if kind == "slotted" else 0)
    return {"sc": sc, "sd": sd, "caps": caps, "rd": rd, "se": se, "re": re_}


def receivers_differ(size: int, seed: int, kind: str = "packed") -> bool:
    """some receiver gets different counts from different senders (its capacities and displacements are no uniform stride), and some
    sender gives different counts to different receivers: a count taken from the wrong peer's box would show"""
    cols = [{count(r, to, seed, size, kind) for r in range(size) if count(r, to, seed, size, kind)} for to in range(size)]
    rows = [{count(frm, j, seed, size, kind) for j in range(size) if count(frm, j, seed, size, kind)} for frm in range(size)]
    return any(len(c) > 1 for c in cols) and any(len(r) > 1 for r in rows)


def expectation(me: int, size: int, seed: int, kind: str, es: int, plans=None, extents=None) -> tuple[np.ndarray, np.ndarray]:
    """(receive buffer + guard as bytes, received counts) of rank `me`"""
    plans = plans or [plan(r, size, seed, kind) for r in range(size)]
    mine = plans[me]
    rb = (extents[me][1] if extents else mine["re"]) * es
    want = np.full(rb + GUARD, FILL, dtype=np.uint8)
    got = np.zeros(size, dtype=np.uint64)
    for r in range(size):
        n = plans[r]["sc"][me]
        got[r] = n
        if n > mine["caps"][r]:
            continue
        src = rank_bytes(r, (extents[r][0] if extents else plans[r]["se"]) * es)
        want[mine["rd"][r] * es:(mine["rd"][r] + n) * es] = src[plans[r]["sd"][me] * es:(plans[r]["sd"][me] + n) * es]
    return want, got


def _hip_runtime():
    return ctypes.CDLL(os.environ.get("XMPI_DEVSIM_LIB") or "libamdhip64.so")


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def v_case(comm, dtype, kind, seed, algo=xmpi.ALGO_AUTO, mem="registered", stream=None, expect=xmpi.OK):
    """one call, checked whole; mem: registered (xmpi_malloc) | host (numpy) | foreign (hipMalloc, never registered);
    stream: the stream-ordered form with the five arrays in device memory"""
    me, size = comm.rank(), comm.size()
    es = xmpi.DTYPE_SIZE[dtype]
    plans = [plan(r, size, seed, kind) for r in range(size)]
    if kind in ("packed", "slotted", "oddbase", "elem") and size > 3:  # (3 ranks: four non-zero pairs, which a seed may make equal)
        assert receivers_differ(size, seed), f"the count matrix of seed {seed} gives every receiver equal counts: it would hide a wrong peer"
    p = plans[me]
    sb, rb = p["se"] * es, p["re"] * es
    mine = rank_bytes(me, sb)
    want, want_counts = expectation(me, size, seed, kind, es, plans)
    what = f"alltoallv {xmpi.DTYPE_NAME[dtype]} {kind} seed={seed} algo={algo} mem={mem} stream={stream is not None} rank {me}/{size}"
    arrays = (_u64(p["sc"]), _u64(p["sd"]), _u64(p["caps"]), _u64(p["rd"]))
    if mem == "host":
        send = mine.copy()
        recv = np.full(rb + GUARD, FILL, dtype=np.uint8)
        got = comm.alltoallv(send, p["se"], arrays[0], arrays[1], recv[:rb], p["re"], arrays[2], arrays[3], dtype, algo)
        assert got.tobytes() == want_counts.tobytes(), f"{what}: counts {got} != {want_counts}"
        bad = np.nonzero(recv != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[0]} of {rb}"
        assert send.tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
        return
    hip = None
    if mem == "foreign":
        hip = _hip_runtime()
        s, r = ctypes.c_void_p(0), ctypes.c_void_p(0)
        comm.sync()
        assert hip.hipMalloc(ctypes.byref(s), ctypes.c_size_t(max(sb, 16))) == 0
        assert hip.hipMalloc(ctypes.byref(r), ctypes.c_size_t(rb + GUARD)) == 0
        sp, rp = s.value, r.value
    else:
        send, recv = comm.alloc(max(sb, 16)), comm.alloc(rb + GUARD)
        sp, rp = send.ptr, recv.ptr
    wantd = comm.alloc(rb + GUARD).upload(want)
    if sb:
        comm.memcpy(sp, mine.ctypes.data, sb)
    comm.memset(rp, FILL, rb + GUARD)
    if stream is not None:
        dev = [comm.alloc(8 * size).upload(a) for a in arrays] + [comm.alloc(8 * size).upload(np.full(size, 2 ** 40, dtype=np.uint64))]
        comm.alltoallv_on_stream(sp, p["se"], dev[0], dev[1], rp, p["re"], dev[2], dev[3], dev[4], dtype, stream)
        comm.stream_sync(stream)
        got = dev[4].download(np.uint64, size)
        for d in dev:
            d.free()
    else:
        got = comm.alltoallv(sp, p["se"], arrays[0], arrays[1], rp, p["re"], arrays[2], arrays[3], dtype, algo)
    assert got.tobytes() == want_counts.tobytes(), f"{what}: counts {got} != {want_counts}"
    bad = comm.count_mismatch(rp, wantd, rb + GUARD)  # (the whole buffer, its gaps and the bytes behind it, on the device)
    if bad:
        out = np.empty(rb + GUARD, dtype=np.uint8)
        comm.memcpy(out.ctypes.data, rp, rb + GUARD)
        idx = np.nonzero(out != want)[0]
        raise AssertionError(f"{what}: {bad} bytes differ, first at byte {idx[0] if idx.size else -1} of {rb}")
    if sb:
        back = np.empty(sb, dtype=np.uint8)
        comm.memcpy(back.ctypes.data, sp, sb)
        assert back.tobytes() == mine.tobytes(), f"{what}: the send buffer was modified"
    wantd.free()
    if hip is not None:
        comm.barrier()
        assert hip.hipFree(s) == 0 and hip.hipFree(r) == 0
    else:
        send.free()
        recv.free()


def _kinds(dtype):
    return LAYOUTS if dtype == xmpi.U8 else ("packed", "slotted", "skewed")


def sc_layouts(comm, args):
    """every layout on U8, F16, I64, blocking, by AUTO / ZCOPY / DIRECT; dsync_v_launches says which path ran"""
    device = bool(comm.get_param("dsync")) and not args.get("expect_host")
    assert comm.size() < 3 or all(receivers_differ(comm.size(), 5 + dtype) for dtype in DTYPES), "every receiver gets equal counts"
    for dtype in DTYPES:
        for kind in _kinds(dtype):
            for algo in args.get("algos", list(ALGOS)):
                before = comm.get_param("dsync_v_launches")
                v_case(comm, dtype, kind, 5 + dtype, algo)
                ran = comm.get_param("dsync_v_launches") - before
                on_dev = device and algo != xmpi.ALGO_DIRECT and (algo == xmpi.ALGO_ZCOPY or comm.get_param("zero_copy"))
                assert ran == (1 if on_dev else 0), f"algo {algo}: {ran} kernel launches with the counts on the device, device path expected: {on_dev}"
    if args.get("expect_host"):
        assert comm.get_param("dsync_v_launches") == 0


def sc_equal(comm, args):
    """equal counts: byte for byte what xmpi_alltoall gives for the same data"""
    me, size = comm.rank(), comm.size()
    for dtype, n in ((xmpi.U8, 4099), (xmpi.I64, 1000), (xmpi.F16, 17)):
        es = xmpi.DTYPE_SIZE[dtype]
        v_case(comm, dtype, "equal", n)
        send, a, b = comm.alloc(size * n * es), comm.alloc(size * n * es), comm.alloc(size * n * es)
        send.upload(rank_bytes(me, size * n * es))
        comm.alltoall(send, a, n, dtype, xmpi.ALGO_ZCOPY)
        p = plan(me, size, n, "equal")
        comm.alltoallv(send, p["se"], _u64(p["sc"]), _u64(p["sd"]), b, p["re"], _u64(p["caps"]), _u64(p["rd"]), dtype)
        assert comm.count_mismatch(a, b, size * n * es) == 0, f"equal counts, dtype {dtype}: differs from xmpi_alltoall"
        for x in (send, a, b):
            x.free()


def sc_memory(comm, args):
    """host slices, device memory nobody registered, the stream form with its arrays in device memory"""
    for mem in ("host", "foreign"):
        for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_DIRECT):
            v_case(comm, xmpi.I64, "slotted", 11, algo, mem=mem)
            v_case(comm, xmpi.U8, "oddbase", 12, algo, mem=mem)
    if comm.get_param("dsync"):
        st = comm.stream_create()
        for dtype in DTYPES:
            for kind in _kinds(dtype):
                v_case(comm, dtype, kind, 21 + dtype, stream=st)
        v_case(comm, xmpi.F16, "slotted", 23, stream=st, mem="foreign")
        comm.stream_destroy(st)


def sc_graph(comm, args):
    """a captured graph replayed 3 times, a different count matrix written into the device arrays before each replay.  What is
    captured is a single chain on one stream."""
    me, size = comm.rank(), comm.size()
    dtype, es, kind = xmpi.I64, 8, "slotted"
    seeds = (31, 32, 33)
    assert size < 3 or all(receivers_differ(size, s) for s in seeds), "every receiver gets equal counts"
    allp = {s: [plan(r, size, s, kind) for r in range(size)] for s in seeds}
    extents = [(max(allp[s][r]["se"] for s in seeds), max(allp[s][r]["re"] for s in seeds)) for r in range(size)]
    se, re_ = extents[me]
    send, recv = comm.alloc(max(se * es, 16)).upload(rank_bytes(me, se * es)), comm.alloc(re_ * es + GUARD)
    dev = [comm.alloc(8 * size) for _ in range(5)]

    def load(seed):
        p = allp[seed][me]
        for d, a in zip(dev, (p["sc"], p["sd"], p["caps"], p["rd"], [2 ** 40] * size)):
            d.upload(_u64(a))
        comm.memset(recv, FILL, re_ * es + GUARD)

    st = comm.stream_create()
    load(seeds[0])
    comm.barrier()
    comm.alltoallv_on_stream(send, se, dev[0], dev[1], recv, re_, dev[2], dev[3], dev[4], dtype, st)  # (everything mapped before the capture)
    comm.stream_sync(st)
    comm.barrier()
    comm.graph_begin(st)
    comm.alltoallv_on_stream(send, se, dev[0], dev[1], recv, re_, dev[2], dev[3], dev[4], dtype, st)
    graph = comm.graph_end(st)
    before = comm.get_param("dsync_v_launches")
    for rep, seed in enumerate(seeds[::-1]):
        load(seed)
        comm.barrier()  # (nobody's replay stores into a buffer its owner is still filling)
        comm.graph_launch(graph, st)
        comm.stream_sync(st)
        want, want_counts = expectation(me, size, seed, kind, es, allp[seed], extents)
        got = dev[4].download(np.uint64, size)
        assert got.tobytes() == want_counts.tobytes(), f"graph replay {rep}: counts {got} != {want_counts}"
        out = recv.download(np.uint8, re_ * es + GUARD)
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, f"graph replay {rep}: {bad.size} bytes differ, first at {bad[0]}"
        comm.barrier()
    assert comm.get_param("dsync_v_launches") == before, "a replay is no call into the library"
    comm.graph_destroy(graph)
    comm.stream_destroy(st)
    for x in [send, recv] + dev:
        x.free()


def sc_back_to_back(comm, args):
    """40 calls back to back without barriers, alternating with xmpi_alltoall (LL) and xmpi_allreduce: the v-boxes are
    single-buffered and rewritten at the next call"""
    me, size = comm.rank(), comm.size()
    n = 64
    a2a_s, a2a_r = comm.alloc(size * n * 4), comm.alloc(size * n * 4)
    ar_s, ar_r = comm.alloc(n * 4), comm.alloc(n * 4)
    ins = [np.arange(size * n, dtype=np.int32) * (r + 3) for r in range(size)]
    a2a_s.upload(ins[me])
    ar_s.upload(ins[me][:n])
    for k in range(40):
        if k % 3 == 0 or k % 3 == 2:
            v_case(comm, (xmpi.U8, xmpi.I64)[k % 2], ("packed", "slotted")[(k // 3) % 2], 40 + k, xmpi.ALGO_AUTO)
        if k % 3 == 1:
            comm.alltoall(a2a_s, a2a_r, n, xmpi.I32, xmpi.ALGO_LL)
            want = np.concatenate([ins[r][me * n:(me + 1) * n] for r in range(size)])
            assert a2a_r.download(np.int32, size * n).tobytes() == want.tobytes(), f"call {k}: alltoall"
        if k % 3 == 2:
            comm.allreduce(ar_s, ar_r, n, xmpi.I32, xmpi.SUM)
            want = sum(x[:n].astype(np.int64) for x in ins).astype(np.int32)
            assert ar_r.download(np.int32, n).tobytes() == want.tobytes(), f"call {k}: allreduce"
    for x in (a2a_s, a2a_r, ar_s, ar_r):
        x.free()


def _raw(comm, send, se, p, recv, re_, dtype, algo=xmpi.ALGO_AUTO):
    got = np.zeros(comm.size(), dtype=np.uint64)
    a = [_u64(p[k]) for k in ("sc", "sd", "caps", "rd")]
    rc = xmpi.lib().xmpi_alltoallv(comm.handle, xmpi._ptr(send), se, a[0].ctypes.data, a[1].ctypes.data, xmpi._ptr(recv), re_,
                                   a[2].ctypes.data, a[3].ctypes.data, got.ctypes.data, dtype, algo)
    return rc, got, xmpi.lib().xmpi_last_error().decode(errors="replace")


def sc_errors(comm, args):
    """error paths (virtual devices only): a pair over capacity, a row out of its extents, then a clean call"""
    me, size = comm.rank(), comm.size()
    algo = args.get("algo", xmpi.ALGO_AUTO)
    dtype, es, n = xmpi.I32, 4, 1000
    a, b = 0, size - 1  # the pair a -> b is over capacity
    data = rank_bytes(me, size * n * es)
    send, recv = comm.alloc(size * n * es).upload(data), comm.alloc(size * n * es + GUARD)
    base = {"sc": [n] * size, "sd": [j * n for j in range(size)], "caps": [n] * size, "rd": [r * n for r in range(size)]}
    # -- truncation
    p = {k: list(v) for k, v in base.items()}
    if me == b:
        p["caps"][a] = n - 1
    comm.memset(recv, FILL, size * n * es + GUARD)
    rc, got, text = _raw(comm, send, size * n, p, recv, size * n, dtype, algo)
    if me in (a, b):
        assert rc == xmpi.ERR_TRUNCATE, f"rank {me}: {rc} ({text}) instead of XMPI_ERR_TRUNCATE"
        assert f"rank {b if me == a else a}" in text, text
    else:
        assert rc == xmpi.OK, f"rank {me}: {rc} ({text}): only the two ranks of the pair see the truncation"
    assert list(got) == [n] * size, f"rank {me}: recvcounts {got}: the offered count is reported"
    want = np.full(size * n * es + GUARD, FILL, dtype=np.uint8)
    for r in range(size):
        if not (me == b and r == a):
            want[r * n * es:(r + 1) * n * es] = rank_bytes(r, size * n * es)[me * n * es:(me + 1) * n * es]
    out = recv.download(np.uint8, size * n * es + GUARD)
    assert out.tobytes() == want.tobytes(), f"rank {me}: after a truncated pair the slot stays as it was and every other block is delivered"
    # -- the next call succeeds
    comm.memset(recv, FILL, size * n * es + GUARD)
    rc, got, text = _raw(comm, send, size * n, base, recv, size * n, dtype, algo)
    assert rc == xmpi.OK and list(got) == [n] * size, (rc, text, got)
    # -- a row that leaves the extent: rank 1's row for rank 0
    p = {k: list(v) for k, v in base.items()}
    if me == 1:
        p["sd"][0] = size * n - 1  # (+ n elements: past the send extent)
    comm.memset(recv, FILL, size * n * es + GUARD)
    rc, got, text = _raw(comm, send, size * n, p, recv, size * n, dtype, algo)
    if me == 1:
        assert rc == xmpi.ERR_ARG and "rank 0" in text, f"rank 1: {rc} ({text}) instead of XMPI_ERR_ARG naming rank 0"
    else:
        assert rc == xmpi.OK, f"rank {me}: {rc} ({text})"
    want = np.full(size * n * es + GUARD, FILL, dtype=np.uint8)
    for r in range(size):
        if {me, r} != {0, 1}:  # (nothing moves between the two, in either direction)
            want[r * n * es:(r + 1) * n * es] = rank_bytes(r, size * n * es)[me * n * es:(me + 1) * n * es]
    out = recv.download(np.uint8, size * n * es + GUARD)
    assert out.tobytes() == want.tobytes(), f"rank {me}: a row out of its extents: nothing written outside, the other pairs delivered"
    assert send.download(np.uint8, size * n * es).tobytes() == data.tobytes()
    # -- the communicator is still usable, by every collective
    comm.memset(recv, FILL, size * n * es + GUARD)
    comm.alltoall(send, recv, n, dtype, xmpi.ALGO_ZCOPY)
    rc, got, text = _raw(comm, send, size * n, base, recv, size * n, dtype, algo)
    assert rc == xmpi.OK, (rc, text)
    # -- from the arguments alone
    rc, _, text = _raw(comm, send, size * n, base, send.ptr + 4, size * n - 1, dtype, algo)
    assert rc == xmpi.ERR_ARG and "overlap" in text, (rc, text)
    for bad in (xmpi.ALGO_RING, xmpi.ALGO_LL, xmpi.ALGO_ZPUSH, 99):
        rc, _, text = _raw(comm, send, size * n, base, recv, size * n, dtype, bad)
        assert rc == xmpi.ERR_UNSUPPORTED and "alltoallv has no" in text, (bad, rc, text)
    send.free()
    recv.free()


def sc_stream_errors(comm, args):
    """the stream form's verdicts arrive with the xmpi_stream_sync behind it; arrays the device cannot address are refused"""
    me, size = comm.rank(), comm.size()
    L = xmpi.lib()
    dtype, es, n = xmpi.I32, 4, 500
    a, b = 0, size - 1
    send, recv = comm.alloc(size * n * es).upload(rank_bytes(me, size * n * es)), comm.alloc(size * n * es + GUARD)
    base = {"sc": [n] * size, "sd": [j * n for j in range(size)], "caps": [n] * size, "rd": [r * n for r in range(size)]}
    dev = [comm.alloc(8 * size) for _ in range(5)]
    st = comm.stream_create()

    def run(p):
        for d, arr in zip(dev, (p["sc"], p["sd"], p["caps"], p["rd"], [2 ** 40] * size)):
            d.upload(_u64(arr))
        comm.memset(recv, FILL, size * n * es + GUARD)
        comm.barrier()
        comm.alltoallv_on_stream(send, size * n, dev[0], dev[1], recv, size * n, dev[2], dev[3], dev[4], dtype, st)
        rc = L.xmpi_stream_sync(comm.handle, st)
        return rc, L.xmpi_last_error().decode(errors="replace"), list(dev[4].download(np.uint64, size))

    # pageable host arrays: from the arguments, before anything is launched
    host = [_u64(base[k]) for k in ("sc", "sd", "caps", "rd")] + [np.zeros(size, dtype=np.uint64)]
    rc = L.xmpi_alltoallv_on_stream(comm.handle, send.ptr, size * n, *[x.ctypes.data for x in host[:2]], recv.ptr, size * n,
                                    *[x.ctypes.data for x in host[2:]], dtype, st)
    assert rc == xmpi.ERR_ARG and "pinned" in L.xmpi_last_error().decode(), (rc, L.xmpi_last_error())
    rc = L.xmpi_alltoallv_on_stream(comm.handle, send.ptr, size * n, dev[0].ptr, dev[1].ptr, recv.ptr, size * n, dev[2].ptr, dev[3].ptr,
                                    host[4].ctypes.data, dtype, st)
    assert rc == xmpi.ERR_ARG, rc
    # a pair over capacity
    p = {k: list(v) for k, v in base.items()}
    if me == b:
        p["caps"][a] = n - 1
    rc, text, got = run(p)
    assert rc == (xmpi.ERR_TRUNCATE if me in (a, b) else xmpi.OK), f"rank {me}: stream_sync gave {rc} ({text})"
    assert got == [n] * size, got
    want = np.full(size * n * es + GUARD, FILL, dtype=np.uint8)
    for r in range(size):
        if not (me == b and r == a):
            want[r * n * es:(r + 1) * n * es] = rank_bytes(r, size * n * es)[me * n * es:(me + 1) * n * es]
    assert recv.download(np.uint8, size * n * es + GUARD).tobytes() == want.tobytes(), f"rank {me}: truncated pair, stream form"
    # a row out of its extents: the last rank's row for rank 0
    p = {k: list(v) for k, v in base.items()}
    if me == b:
        p["rd"][a] = size * n - 1
    rc, text, got = run(p)
    assert rc == (xmpi.ERR_ARG if me == b else xmpi.OK), f"rank {me}: stream_sync gave {rc} ({text})"
    # the verdict was consumed: a clean call, and a blocking collective behind it, succeed
    rc, text, got = run(base)
    assert rc == xmpi.OK and got == [n] * size, (rc, text, got)
    comm.allreduce(send, recv, n, dtype, xmpi.SUM)
    comm.stream_destroy(st)
    for x in [send, recv] + dev:
        x.free()


def sc_mismatch(comm, args):
    """rank 0 calls xmpi_alltoall instead, over the same bytes: every rank gets "not in the same call", nothing moved"""
    me, size = comm.rank(), comm.size()
    n = 20000  # (above the LL lines' limit: the fold announces its call)
    send, recv = comm.alloc(size * n * 4), comm.alloc(size * n * 4)
    comm.memset(recv, FILL, size * n * 4)
    p = plan(me, size, n, "equal")
    if me == 0:
        rc = xmpi.lib().xmpi_alltoall(comm.handle, send.ptr, recv.ptr, n, xmpi.I32, xmpi.ALGO_ZCOPY)
        text = xmpi.lib().xmpi_last_error().decode()
    else:
        rc, _, text = _raw(comm, send, p["se"], p, recv, p["re"], xmpi.I32, xmpi.ALGO_ZCOPY)
    assert rc == xmpi.ERR_ARG and "not in the same call" in text, (me, rc, text)
    assert np.all(recv.download(np.uint8, size * n * 4) == FILL), "something was moved"
    print("vcoll mismatch: ok", flush=True)
    os._exit(0)  # (the job is aborted: nothing more can be done on this communicator, finalize included)


SCENARIOS = {"layouts": sc_layouts, "equal": sc_equal, "memory": sc_memory, "graph": sc_graph, "back_to_back": sc_back_to_back,
             "errors": sc_errors, "stream_errors": sc_stream_errors, "mismatch": sc_mismatch}
