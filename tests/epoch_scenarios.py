"""Scenarios that run the device counters across their 32-bit edges.  The collectives and the stream-ordered Send / Receive order
themselves by an epoch the kernels count (64 bits, DsyncPage::epoch_now), by the communicator's number (the epoch it was born at, plus
one) and by a message number per ordered pair; the LL lines carry the low 32 bits of the epoch as their flag.  A job reaches epoch
2^32 after hours -- so the test-only variables XMPI_TEST_EPOCH_BASE (the communicator is born as if its pages had seen that many
epochs) and XMPI_TEST_P2P_SEQ0 (... and every pair had exchanged that many messages) start the counters next to the edge.

Each function runs on ONE rank (tests/epoch_worker.py); every result is compared bit for bit with the oracle (oracle.*, numpy):
I64 sums and F32 folds in rank order are exact or order-defined.  Every job runs with XMPI_TIMEOUT_S of a few seconds: a wait that never
matches ends as XMPI_ERR_TIMEOUT, not as a hang."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from mpi_amd import xmpi
from oracle import oracle
from tests import personal_scenarios as ps
from tests import vcoll_scenarios as vs
from tests.scenarios import allgather_case, allreduce_case, bcast_case, np_hash, reduce_case

K = 8  # kP2PBoxes (mpi_amd/csrc/kernels.h): messages in flight per ordered pair
COUNTERS = ("dsync_launches", "dsync_ll_launches", "dsync_ll_agent", "dsync_split_launches", "dsync_sched_launches", "dsync_v_launches")
L, Z = xmpi.ALGO_LL, xmpi.ALGO_ZCOPY
MID = 4099  # elements of the calls that are not LL lines: 16 KiB of F32, 32 KiB + 24 of I64 -- above every LL limit a job chooses or is given


def edge_of(base: int) -> int:
    """the next multiple of 2^31 above `base`: where a 32-bit reading of the epoch changes sign or wraps"""
    return ((base >> 31) + 1) << 31


def _hip():
    return ctypes.CDLL(os.environ.get("XMPI_DEVSIM_LIB") or "libamdhip64.so")


def _counters(comm):
    return {k: comm.get_param(k) for k in COUNTERS}


def _delta(comm, before):
    return {k: comm.get_param(k) - v for k, v in before.items()}


# ---- one call of every form, each confirmed by the launch counters --------------------------------------------------------------------
def _is_ll(d):
    return d["dsync_ll_launches"] == 1 and d["dsync_ll_agent"] == 0 and d["dsync_launches"] >= 1 and d["dsync_sched_launches"] == 0


def _is_agent(d):
    return d["dsync_ll_launches"] == 1 and d["dsync_ll_agent"] == 1


def _is_fold(d):
    return d["dsync_launches"] == 1 and d["dsync_split_launches"] == 0 and d["dsync_ll_launches"] == 0 and d["dsync_sched_launches"] == 0


def _is_split(d):
    return d["dsync_split_launches"] == 1 and d["dsync_launches"] == 3 and d["dsync_ll_launches"] == 0


def _is_stepped(d):
    return d["dsync_sched_launches"] == 1 and d["dsync_ll_launches"] == 0


def _not_ll(d):  # a fold of a collective whose launch count is its own business: no LL lines, no stepped kernel
    return d["dsync_ll_launches"] == 0 and d["dsync_sched_launches"] == 0 and d["dsync_launches"] >= 1


def _is_v(d):
    return d["dsync_v_launches"] == 1


def _forms(comm):
    """(what, parameters, the call, what the counters must say) of every form cross() runs: LL launched at 8 B, 1 KiB and the largest
    payload; the one-kernel fold and meet / body / done; ring, halving + doubling and tree in pull and push form; allgather, bcast and
    reduce from the last rank, reduce-scatter and all-to-all as LL lines and as a fold; alltoallv"""
    size = comm.size()
    maxb = comm.get_param("ll_max_bytes")
    last = size - 1
    ll_off = {"agent_ll": 0}
    one = {"dsync_split_bytes": 0}
    split = {"dsync_split_bytes": 1, "body_sys": 0}
    f = [("LL launched, 8 B", ll_off, lambda: allreduce_case(comm, xmpi.I64, 1, L, exact=True), _is_ll),
         ("LL launched, 1 KiB", ll_off, lambda: allreduce_case(comm, xmpi.F32, 256, L, exact=True), _is_ll),
         ("LL launched, the largest payload", ll_off, lambda: allreduce_case(comm, xmpi.I64, maxb // 8, L, exact=True), _is_ll),
         ("fold, one kernel", one, lambda: allreduce_case(comm, xmpi.F32, MID, Z, exact=True), _is_fold),
         ("fold, one kernel, I64", one, lambda: allreduce_case(comm, xmpi.I64, MID, Z, exact=True), _is_fold),
         ("fold, meet / body / done", split, lambda: allreduce_case(comm, xmpi.F32, MID, Z, exact=True), _is_split),
         ("fold, meet / body / done, I64", split, lambda: allreduce_case(comm, xmpi.I64, MID, Z, exact=True), _is_split)]
    for what, algo in (("ring, pull", xmpi.ALGO_RING), ("ring, push", xmpi.ALGO_RING_PUSH), ("halving, pull", xmpi.ALGO_RHD), ("halving, push", xmpi.ALGO_RHD_PUSH)):
        f.append((what, {}, lambda algo=algo: allreduce_case(comm, xmpi.I64, MID, algo, exact=True), _is_stepped))
    for what, algo in (("tree, pull", xmpi.ALGO_TREE), ("tree, push", xmpi.ALGO_TREE_PUSH)):
        f.append((what, {}, lambda algo=algo: reduce_case(comm, xmpi.I64, MID, last, algo, pat=xmpi.PAT_UNIFORM, what=what), _is_stepped))
    f += [("allgather, LL", ll_off, lambda: allgather_case(comm, xmpi.I64, 100, L), _is_ll),
          ("allgather, fold", one, lambda: allgather_case(comm, xmpi.I64, MID, Z), _not_ll),
          ("bcast from the last rank, LL", ll_off, lambda: bcast_case(comm, xmpi.I64, 100, last, L), _is_ll),
          ("bcast from the last rank, fold", one, lambda: bcast_case(comm, xmpi.I64, MID, last, Z), _not_ll),
          ("reduce to the last rank, LL", ll_off, lambda: reduce_case(comm, xmpi.F32, 1001, last, L), _is_ll),
          ("reduce to the last rank, fold", one, lambda: reduce_case(comm, xmpi.F32, MID, last, Z), _not_ll),
          ("reduce-scatter, LL", ll_off, lambda: ps.personal_case(comm, ps.RS, xmpi.F32, 100, L), _is_ll),
          ("reduce-scatter, fold", one, lambda: ps.personal_case(comm, ps.RS, xmpi.I64, MID, Z), _not_ll),
          ("all-to-all, LL", ll_off, lambda: ps.personal_case(comm, ps.A2A, xmpi.I64, 100, L), _is_ll),
          ("all-to-all, fold", one, lambda: ps.personal_case(comm, ps.A2A, xmpi.I64, MID, Z), _not_ll),
          ("alltoallv, packed", {}, lambda: vs.v_case(comm, xmpi.I64, "packed", 31, Z), _is_v),
          ("alltoallv, skewed", {}, lambda: vs.v_case(comm, xmpi.I64, "skewed", 32, Z), _is_v)]
    return f


def run_form(comm, form):
    what, params, call, ran = form
    old = {k: comm.get_param(k) for k in params}
    for k, v in params.items():
        comm.set_param(k, v)
    before = _counters(comm)
    call()
    d = _delta(comm, before)
    assert ran(d), f"{what}: another form ran: the counters moved by {d} (epoch {comm.get_param('dsync_epoch')})"
    for k, v in old.items():
        comm.set_param(k, v)
    return 1


def agent_runs(comm):
    """LL by the agent: a run of consecutive agent calls (the agent counts prev_epoch + 1 without reading the page), a launched kernel
    in between (the next call tells the agent to read the page again), at 8 B, 1 KiB and the largest payload.  x -> size^k x in I64
    (wraps like Go): one wrong or repeated contribution anywhere shows in the end.  Returns the calls made."""
    size = comm.size()
    assert comm.get_param("agent_ll") >= 1 and comm.get_param("ll_agent_us") > 0, "the LL agent is off in this job: the form cannot be forced"
    maxb = comm.get_param("ll_max_bytes")
    ab = comm.get_param("agent_ll_bytes")
    comm.set_param("agent_ll_bytes", maxb)
    served = lambda: comm.get_param("dsync_ll_agent")
    st = comm.stream_create()
    n = 0
    for m in (1, 128, maxb // 8):
        a, b = comm.alloc(m * 8), comm.alloc(m * 8)
        comm.fill(a, m, xmpi.I64, xmpi.PAT_CONST, 0)  # all ones
        comm.sync()
        g0 = served()
        for _ in range(3):
            comm.allreduce(a, b, m, xmpi.I64, xmpi.SUM, L)
            comm.allreduce(b, a, m, xmpi.I64, xmpi.SUM, L)
        assert served() == g0 + 6, f"consecutive blocking LL collectives of {m * 8} bytes: {served() - g0} of 6 by the agent"
        comm.allreduce_on_stream(a, b, m, xmpi.I64, xmpi.SUM, st)  # launched: size^7
        comm.stream_sync(st)
        comm.sync()  # (the agent takes a call only when it finds the streams idle: the library asks hipStreamQuery)
        comm.allreduce(b, a, m, xmpi.I64, xmpi.SUM, L)             # the agent, told to read the epoch: size^8
        comm.allreduce(a, b, m, xmpi.I64, xmpi.SUM, L)             # ... and to count again: size^9
        comm.bcast(b, m, xmpi.I64, size - 1, L)
        comm.allreduce(b, a, m, xmpi.I64, xmpi.SUM, L)             # size^10
        assert served() == g0 + 10, f"the agent behind a launched kernel ({m * 8} bytes): {served() - g0} of 10 calls"
        with np.errstate(over="ignore"):
            want = np.uint64(size) ** np.uint64(10)
        assert np.all(a.download(np.int64, m).view(np.uint64) == want), f"LL by the agent, {m * 8} bytes: epochs counted by the agent, a launched kernel in between"
        a.free()
        b.free()
        n += 11
    comm.stream_destroy(st)
    comm.set_param("agent_ll_bytes", ab)
    return n


# ---- stream-ordered Send / Receive -----------------------------------------------------------------------------------------------------
def _payload(src, dst, k, seed):
    """message k of src -> dst: its length, tag and words are all hashes of (seed, src, dst, k) -- a swapped, repeated or stale message differs"""
    s = seed * 1000003 + src * 10007 + dst * 101 + k
    n = 1 + int(np_hash(s, np.zeros(1, dtype=np.uint64))[0] % np.uint64(700))
    return np_hash(s + 1, np.arange(n, dtype=np.uint64)).view(np.int64), 40 + (k & 1)  # (tags alternate)


NMAX = 700


def exchange(comm, peers, m, seed, st):
    """m messages in each direction between this rank and every rank of `peers`, all on stream `st`, in batches of kP2PBoxes with a
    stream_sync behind each.  Every rank walks its pairs in the order of (lower rank, higher rank), the lower rank of a pair sends first:
    no stream waits for work queued behind it.  Every payload, length (the words behind it keep their fill) and tag is checked."""
    me = comm.rank()
    slot = NMAX * 8
    sbuf, rbuf = comm.alloc(m * slot), comm.alloc(m * slot + 8)
    for peer in sorted(peers):
        out = [_payload(me, peer, k, seed) for k in range(m)]
        inn = [_payload(peer, me, k, seed) for k in range(m)]
        image = np.zeros(m * NMAX, dtype=np.int64)
        for k, (p, _) in enumerate(out):
            image[k * NMAX:k * NMAX + p.size] = p
        sbuf.upload(image)
        comm.memset(rbuf, 0xA5, m * slot + 8)
        comm.sync()
        for phase in ((0, 1) if me < peer else (1, 0)):
            for k0 in range(0, m, K):
                for k in range(k0, min(k0 + K, m)):
                    if phase == 0:
                        comm.send_on_stream(sbuf.at(k * slot), out[k][0].size, xmpi.I64, peer, out[k][1], st)
                    else:
                        comm.recv_on_stream(rbuf.at(k * slot), NMAX, xmpi.I64, peer, inn[k][1], st)
                comm.stream_sync(st)
        got = rbuf.download(np.int64, m * NMAX)
        fill = np.int64(np.uint64(0xA5A5A5A5A5A5A5A5).astype(np.int64))
        for k, (p, tag) in enumerate(inn):
            g = got[k * NMAX:(k + 1) * NMAX]
            assert g[:p.size].tobytes() == p.tobytes(), f"message {k} of {peer} -> {me} (tag {tag}, {p.size} words): another payload arrived"
            assert np.all(g[p.size:] == fill), f"message {k} of {peer} -> {me} (tag {tag}): more than its {p.size} words were written"
        assert sbuf.download(np.int64, m * NMAX).tobytes() == image.tobytes(), "a send buffer was modified"
    sbuf.free()
    rbuf.free()
    return 2 * m * len(peers)


def ring_exchange(comm, m, seed, st):
    me, size = comm.rank(), comm.size()
    return exchange(comm, {(me + 1) % size, (me - 1) % size}, m, seed, st)


def late_receive(comm, st):
    """rank 0 sends to rank 1, which posts its Receive late: behind a barrier over the host control block that rank 0 enters only after it
    has read -- from a word its stream writes behind the Send -- that the Send has not completed.  Behind the Send the stream also
    overwrites the payload (a completed Send says the buffer is free): a Send that completed early is seen by the receiver as well."""
    me = comm.rank()
    n = 2000
    want = np_hash(991, np.arange(n, dtype=np.uint64)).view(np.int64)
    if me == 0:
        hip = _hip()
        buf, one = comm.alloc(n * 8).upload(want), comm.alloc(8).upload(np.array([1], dtype=np.int64))
        word = ctypes.c_void_p(0)  # pinned host memory: read below without any work on the GPU
        assert hip.hipHostMalloc(ctypes.byref(word), ctypes.c_size_t(64), 0) == 0
        done = ctypes.c_int64.from_address(word.value)
        done.value = 0
        comm.sync()
        comm.send_on_stream(buf, n, xmpi.I64, 1, 77, st)
        assert hip.hipMemsetAsync(ctypes.c_void_p(buf.ptr), 0x5C, ctypes.c_size_t(n * 8), ctypes.c_void_p(st)) == 0
        assert hip.hipMemcpyAsync(word, ctypes.c_void_p(one.ptr), ctypes.c_size_t(8), 4, ctypes.c_void_p(st)) == 0  # (hipMemcpyDefault)
        comm.barrier()  # the receiver is known not to have posted its Receive before this one ...
        early = done.value
        comm.barrier()  # ... nor before this one, which rank 0 enters with the word read
        assert early == 0, "the Send's stream went on before the Receive was posted: a Send completed that nobody had consumed"
        comm.stream_sync(st)
        assert done.value == 1
        assert hip.hipHostFree(word) == 0
        buf.free()
        one.free()
    else:
        comm.barrier()
        comm.barrier()
        if me == 1:
            rbuf = comm.alloc(n * 8)
            comm.memset(rbuf, 0, n * 8)
            comm.recv_on_stream(rbuf, n, xmpi.I64, 0, 77, st)
            comm.stream_sync(st)
            assert rbuf.download(np.int64, n).tobytes() == want.tobytes(), "the late Receive got a payload its sender had already overwritten"
            rbuf.free()
    comm.barrier()


# ---- the scenarios ----------------------------------------------------------------------------------------------------------------------
def graph_on_the_edge(comm, edge, st):
    """a captured graph of two LL collectives, replayed four times from epoch edge - 3 (or from where the communicator stands, if that
    is later): one replay ends exactly on `edge` and the next begins on edge + 1 -- where `edge` is a multiple of 2^32 their flags are
    both 1 and only the slot's parity tells the lines apart.  New inputs for every replay.  Returns the first replay's first epoch and how many epochs the replays took."""
    me, size = comm.rank(), comm.size()
    m = 128  # 1 KiB: LL lines under every limit
    a, b = comm.alloc(m * 8), comm.alloc(m * 8)
    agent_ll = comm.get_param("agent_ll")
    comm.set_param("agent_ll", 0)
    first = comm.get_param("dsync_epoch") + 1
    assert edge - 3 <= first <= edge, f"the replays do not reach epoch {edge} from {first}"
    comm.sync()
    comm.barrier()
    before = _counters(comm)
    comm.graph_begin(st)
    comm.allreduce_on_stream(a, b, m, xmpi.I64, xmpi.SUM, st)
    comm.bcast_on_stream(b, m, xmpi.I64, size - 1, st)
    graph = comm.graph_end(st)
    assert _delta(comm, before)["dsync_ll_launches"] == 2, "the captured collectives are not LL lines"
    for rep in range(4):
        ins = [oracle.fill(m, xmpi.I64, xmpi.PAT_UNIFORM, 7100 + 10 * rep + r) for r in range(size)]
        a.upload(ins[me])
        comm.memset(b, 0xA5, m * 8)
        comm.barrier()  # (nobody's replay reads a buffer its owner is still filling)
        comm.graph_launch(graph, st)
        comm.stream_sync(st)
        want = oracle.reduce_ranks(ins, xmpi.I64, xmpi.SUM)
        assert b.download(np.int64, m).tobytes() == want.tobytes(), f"graph replay {rep} (epochs {first + 2 * rep}, {first + 2 * rep + 1}; the edge is {edge})"
        comm.barrier()
    comm.graph_destroy(graph)
    comm.set_param("agent_ll", agent_ll)
    a.free()
    b.free()
    return first, 8


def pad_to(comm, epoch):
    """launched 8 B LL allreduces until the communicator stands at `epoch` (if it is not there or beyond already)"""
    agent_ll, n = comm.get_param("agent_ll"), 0
    comm.set_param("agent_ll", 0)
    while comm.get_param("dsync_epoch") < epoch:
        allreduce_case(comm, xmpi.I64, 1, L, exact=True)
        n += 1
    comm.set_param("agent_ll", agent_ll)
    return n


def sc_cross(comm, args):
    """one sequence of calls whose epochs straddle edge_of(base): what fits below the edge of every form (tests/epoch_scenarios.py _forms,
    agent_runs), the captured graph on the edge itself, then every form, the agent's runs and a ring of Send / Receive above it.
    args["cover"] (a job whose calls are slow: 8 processes on one GPU): one call of each form above the edge, none below."""
    me, size = comm.rank(), comm.size()
    base = int(args["base"])
    edge = edge_of(base)
    assert comm.get_param("dsync") == 1 and comm.get_param("dsync_epoch") == base, f"born at epoch {comm.get_param('dsync_epoch')}, not at {base}"
    cover = bool(args.get("cover"))
    forms = _forms(comm)
    st = comm.stream_create()
    n = 0
    # (a form takes 1 epoch, the agent's runs 33: they start only where they end below the graph's first epoch)
    i = 0
    while not cover and i < len(forms) and comm.get_param("dsync_epoch") + 1 <= edge - 4:
        n += run_form(comm, forms[(i + size) % len(forms)])  # (jobs of different sizes begin with different forms)
        i += 1
    assert comm.get_param("dsync_epoch") < edge, "the epoch was not below the edge before the crossing"
    n += pad_to(comm, edge - 4)
    if args.get("edge_by") == "agent":  # the agent's consecutive calls count prev_epoch + 1 across the edge
        first = comm.get_param("dsync_epoch") + 1
        n += agent_runs(comm)
        true_epoch = comm.get_param("dsync_epoch")
    else:
        first, took = graph_on_the_edge(comm, edge, st)
        n += took
        true_epoch = first + took - 1  # (the host's count does not see replays; it counted the two captured launches)
    assert first <= edge <= true_epoch
    skew = true_epoch - comm.get_param("dsync_epoch")
    for rep in range(1 if cover else 2):
        for form in forms:
            n += run_form(comm, form)
        n += agent_runs(comm)
        n += ring_exchange(comm, 2 * K + 4, 50 + rep, st)
    now = comm.get_param("dsync_epoch") + skew
    assert now >= edge, "the epoch is not above the edge after the crossing"
    assert cover or n >= 64, n
    comm.stream_destroy(st)
    if me == 0:
        print(f"epoch cross: base {base}, edge {edge}: {n} calls checked, epochs {base + 1} .. {now}")


def _comm(comm, key, tag):
    return xmpi.Comm(comm.rank(), comm.size(), comm.device(), f"{key}-{tag}")


def sc_succession(comm, args):
    """communicator A, born just below an edge, runs every form across it, exchanges more than kP2PBoxes messages with every peer (all
    boxes, acks and `taken` words of its page are left with A's numbers) and is finalised; communicator B of the same processes takes the
    same pooled pages, born above the edge -- a number that is SMALLER than A's in its low 32 bits.  B exchanges with every peer, a Send
    is held back by a late Receive, then alltoallv, LL lines and a fold.  args["wrap"]: the job runs with XMPI_TEST_P2P_SEQ0 next to
    2^32, and B's exchange is message_wrap's."""
    me, size = comm.rank(), comm.size()
    base, key = int(args["base"]), args["key"]
    edge = edge_of(base)
    peers = set(range(size)) - {me}
    a = _comm(comm, key, "A")
    assert a.get_param("dsync_epoch") == base, f"A was born at epoch {a.get_param('dsync_epoch')}, not at {base}"
    st = a.stream_create()
    n = 0
    for form in _forms(a):
        n += run_form(a, form)
    n += agent_runs(a)
    while a.get_param("dsync_epoch") < edge + 8:
        allreduce_case(a, xmpi.I64, 1, L, exact=True)
        n += 1
    n += exchange(a, peers, K + 3, 60, st)
    a.stream_destroy(st)
    last_a = a.get_param("dsync_epoch")
    a.barrier()
    a.finalize()
    b = _comm(comm, key, "B")
    born = b.get_param("dsync_epoch")
    assert born > last_a >= edge, f"B was born at epoch {born}: not above what A left in the pooled pages ({last_a})"
    assert (born + 1) & 0xffffffff < (base + 1) & 0xffffffff, "B's number is not below A's in its low 32 bits: the scenario does not test what it says"
    st = b.stream_create()
    n += exchange(b, peers, int(args.get("wrap", 0)) and 40 or K + 3, 61, st)
    late_receive(b, st)
    n += run_form(b, [f for f in _forms(b) if f[0] == "alltoallv, packed"][0])
    n += run_form(b, [f for f in _forms(b) if f[0] == "LL launched, 1 KiB"][0])
    n += run_form(b, [f for f in _forms(b) if f[0] == "fold, one kernel"][0])
    n += exchange(b, peers, K + 3, 62, st)
    b.stream_destroy(st)
    b.barrier()
    b.finalize()
    if me == 0:
        print(f"epoch succession: A {base} .. {last_a}, B born at {born}: {n} calls checked")


def sc_message_wrap(comm, args):
    """XMPI_TEST_P2P_SEQ0 = 2^32 - 16: 40 messages per ordered pair on a stream cross message number 2^32 of every pair"""
    me, size = comm.rank(), comm.size()
    st = comm.stream_create()
    n = exchange(comm, set(range(size)) - {me}, 40, 70, st)
    late_receive(comm, st)
    comm.stream_destroy(st)
    if me == 0:
        print(f"epoch message wrap: {n} messages checked")


def sc_unset(comm, args):
    """both variables unset: a fixed sequence of collectives, and what the launch counters and the epoch say afterwards (the test holds
    them to what the parent commit gave)"""
    for form in _forms(comm):
        run_form(comm, form)
    agent_runs(comm)
    st = comm.stream_create()
    ring_exchange(comm, K + 3, 80, st)
    comm.stream_destroy(st)
    if comm.rank() == 0:
        print("epoch unset counters: " + " ".join(f"{k}={comm.get_param(k)}" for k in COUNTERS + ("dsync_epoch",)))


SCENARIOS = {"cross": sc_cross, "succession": sc_succession, "message_wrap": sc_message_wrap, "unset": sc_unset}
