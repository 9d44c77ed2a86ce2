"""A model of the stream-ordered Send / Receive protocol (mpi_amd/csrc/sched.hip `p2p_send_kernel` / `p2p_recv_kernel`,
mpi_amd/csrc/dsync_p2p.cpp `dsync_send` / `dsync_recv`) that runs on the CPU: kernels are little state machines, streams run
their kernels in order, a seeded random scheduler interleaves everything that can move.

What the real thing keeps in the flag allocations the model keeps in dictionaries:
  box[(src, dst)][b]   {seq, tag, payload}   written by the sender's kernel, b = (n - 1) % K for message number n of the pair
  ack[(src, dst)][b]   seq                   written by the receiver's kernel when it has consumed the message of that box
  taken[(src, dst)][b] seq                   the receiver's own note of the last message it consumed from the box
Every word is 64 bits wide, as in the kernels (the model masks: Python's integers would hide a narrowing).  Two protocols:
  "cleared"  what the kernels do: the pages are pooled, and a communicator clears these three areas of its own page when it connects;
             the message number is the whole word, nothing is packed beside it;
  "packed"   what they did before: nothing cleared, seq = (communicator number, 32 bits) << 32 | n with n taken back out of the low
             32 bits, the communicator number compared for equality and the words for order -- kept so that the tests can show the
             model sees what that did at a 32-bit edge (test_p2p_sim.py: succession, message 2^32).
`seq0`: every ordered pair has exchanged that many messages already, all consumed and answered (XMPI_TEST_P2P_SEQ0).

Checked: every receive gets the payload of the send with its tag (oldest first when a tag repeats); a box is never
overwritten before its message was consumed; a send completes only after its message was consumed; everything terminates
whatever the interleaving -- as long as the program obeys the documented rule (no stream waits for work queued behind it);
stale records of an earlier communicator in the same pages are never matched.  `bugs` switches known-bad variants on."""
from __future__ import annotations

import random

K = 8  # kP2PBoxes
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


class Violation(AssertionError):
    pass


def run(ops, seed=0, comm_tag=1, stale=None, bugs=(), protocol="cleared", seq0=0):
    """ops: {rank: [stream, ...]}, a stream = list of ("send", peer, tag, payload) / ("recv", peer, tag).
    stale: {pair: [(seq, tag) per box]} -- what an earlier communicator left in the pages (consumed and answered, unless
    "stale_unconsumed").  Returns {(rank, stream index, op index): received payload}."""
    assert protocol in ("cleared", "packed")
    packed = protocol == "packed"
    rng = random.Random(seed)
    box, ack, taken = {}, {}, {}
    consumed = set()

    def number(n):  # the word a message number travels as
        return ((((comm_tag & M32) << 32) | n) if packed else n) & M64

    def mine(seq):  # receive side: is this record one of this communicator's?
        return seq >> 32 == comm_tag & M32 if packed and "no_comm_check" not in bugs else True

    def tab(t, pair):
        return t.setdefault(pair, [dict(seq=0, tag=None, payload=None) if t is box else 0 for _ in range(K)])

    if stale:  # what an earlier communicator left behind in the (uncleared) pages
        for pair, recs in stale.items():
            for b, (seq, tag) in enumerate(recs):
                tab(box, pair)[b] = dict(seq=seq, tag=tag, payload="STALE")
                tab(taken, pair)[b] = 0 if "stale_unconsumed" in bugs else seq
                tab(ack, pair)[b] = 0 if "stale_unconsumed" in bugs else seq
    pairs = {(r, op[1]) if op[0] == "send" else (op[1], r) for r, streams in ops.items() for stream in streams for op in stream}
    if not packed and "no_clear" not in bugs:  # connect: every rank clears the boxes, acks and `taken` words of its own page
        box, ack, taken = {}, {}, {}
    if seq0:  # ... or leaves them as seq0 messages per pair, all consumed and answered, leave them
        for pair in pairs:
            for b in range(K):
                last = number(seq0 - (seq0 - 1 - b) % K) if seq0 > b else 0
                tab(box, pair)[b] = dict(seq=last, tag=None, payload="SEEDED")
                tab(taken, pair)[b] = tab(ack, pair)[b] = last
    out_seq = {pair: seq0 for pair in pairs}
    # the host numbers the messages of an ordered pair when it ENQUEUES the send (dsync_send)
    kernels = {}
    for rank, streams in ops.items():
        for si, stream in enumerate(streams):
            for oi, op in enumerate(stream):
                k = dict(rank=rank, op=op, state="new", got=None)
                if op[0] == "send":
                    n = out_seq[(rank, op[1])] = out_seq[(rank, op[1])] + 1
                    k["seq"] = number(n)
                    k["n"] = k["seq"] & M32 if packed else k["seq"]  # (what the kernel takes back out of the word)
                kernels[(rank, si, oi)] = k
    pos = {(rank, si): 0 for rank, streams in ops.items() for si in range(len(streams))}
    results, idle = {}, 0
    while any(pos[(r, si)] < len(ops[r][si]) for (r, si) in pos):
        live = [(r, si) for (r, si) in pos if pos[(r, si)] < len(ops[r][si])]
        r, si = rng.choice(live)
        key = (r, si, pos[(r, si)])
        k = kernels[key]
        op = k["op"]
        moved = True
        if op[0] == "send":
            pair = (r, op[1])
            b = ((k["n"] - 1) & M64) % K
            if k["state"] == "new":
                if k["n"] > K and tab(ack, pair)[b] < (k["seq"] - K) & M64 and "no_box_wait" not in bugs:
                    moved = False  # the message that used the box before has not been answered yet
                else:
                    old = tab(box, pair)[b]
                    if mine(old["seq"]) and old["seq"] > tab(taken, pair)[b]:
                        raise Violation(f"box {b} of {pair} overwritten before message {old['seq'] & 0xffffffff} was consumed")
                    tab(box, pair)[b] = dict(seq=k["seq"], tag=op[2], payload=op[3])
                    k["state"] = "posted"
            elif tab(ack, pair)[b] >= k["seq"]:
                if (pair, k["seq"]) not in consumed:
                    raise Violation(f"the send of message {k['seq'] & M32} of {pair} completed before any receive had consumed it")
                k["state"] = "done"
            else:
                moved = False
        else:
            pair = (op[1], r)
            if k["state"] == "new":
                best = None
                for b in range(K):
                    rec = tab(box, pair)[b]
                    if not mine(rec["seq"]):
                        continue
                    if rec["seq"] == 0 or rec["seq"] <= tab(taken, pair)[b] or rec["tag"] != op[2]:
                        continue
                    if best is None or rec["seq"] < tab(box, pair)[best]["seq"]:
                        best = b
                if best is None:
                    moved = False
                else:
                    rec = tab(box, pair)[best]
                    k["got"], k["b"], k["seq"] = rec["payload"], best, rec["seq"]
                    tab(taken, pair)[best] = rec["seq"]
                    k["state"] = "copied"
            else:
                consumed.add((pair, k["seq"]))
                tab(ack, pair)[k["b"]] = k["seq"]
                results[key] = k["got"]
                k["state"] = "done"
        if k["state"] == "done":
            pos[(r, si)] += 1
        idle = 0 if moved else idle + 1
        if idle > 20000:
            raise Violation("deadlock: no kernel can make progress")
    return results
