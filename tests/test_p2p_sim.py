"""The stream-ordered Send / Receive protocol under random interleavings -- see tests/p2p_sim.py (CPU only)."""
import pytest

from tests import p2p_sim as sim


def test_ping_pong_and_more_messages_than_boxes():
    for seed in range(20):
        # rank 0 sends 30 messages on one stream, rank 1 receives them in order; then the echo
        ops = {0: [[("send", 1, 100 + k, f"m{k}") for k in range(30)] + [("recv", 1, 7)]],
               1: [[("recv", 0, 100 + k) for k in range(30)] + [("send", 0, 7, "echo")]]}
        got = sim.run(ops, seed=seed)
        assert [got[(1, 0, k)] for k in range(30)] == [f"m{k}" for k in range(30)] and got[(0, 0, 30)] == "echo"


def test_concurrent_streams_tags_in_any_order():
    """several streams per rank: messages with distinct tags overtake each other, every receive still gets ITS message"""
    for seed in range(40):
        ops = {0: [[("send", 1, t, f"a{t}")] for t in (1, 2, 3, 4)] + [[("recv", 1, 9)]],
               1: [[("recv", 0, t)] for t in (4, 2, 3, 1)] + [[("send", 0, 9, "z")]]}
        got = sim.run(ops, seed=seed)
        for si, t in enumerate((4, 2, 3, 1)):
            assert got[(1, si, 0)] == f"a{t}"
        assert got[(0, 4, 0)] == "z"


def test_the_same_tag_twice_is_first_come_first_served():
    for seed in range(20):
        ops = {0: [[("send", 1, 5, "first"), ("send", 1, 5, "second")]], 1: [[("recv", 0, 5), ("recv", 0, 5)]]}
        got = sim.run(ops, seed=seed)
        assert (got[(1, 0, 0)], got[(1, 0, 1)]) == ("first", "second")


def test_three_ranks_every_pair():
    for seed in range(20):
        ops = {r: [[("send", p, 10 * r + p, f"{r}->{p}") for p in range(3) if p != r], [("recv", p, 10 * p + r) for p in range(3) if p != r]]
               for r in range(3)}
        got = sim.run(ops, seed=seed)
        for r in range(3):
            assert [got[(r, 1, i)] for i in range(2)] == [f"{p}->{r}" for p in range(3) if p != r]


def test_a_stream_that_waits_for_work_behind_it_deadlocks():
    """the documented rule, shown: a send whose receive is queued BEHIND a receive that needs the peer's later send"""
    ops = {0: [[("send", 1, 1, "x"), ("send", 1, 2, "y")]], 1: [[("recv", 0, 2), ("recv", 0, 1)]]}
    with pytest.raises(sim.Violation, match="deadlock"):
        sim.run(ops, seed=1)


def test_records_of_an_earlier_communicator_are_not_matched():
    """pages are pooled: a box may still hold a message of the communicator before, even one that was never consumed (its job was
    aborted) -- the next communicator clears the boxes of its page when it connects"""
    stale = {(0, 1): [(b + 1, 5) for b in range(sim.K)]}  # the communicator before left 8 messages with tag 5
    for seed in range(10):
        ops = {0: [[("send", 1, 5, "fresh")]], 1: [[("recv", 0, 5)]]}
        got = sim.run(ops, seed=seed, comm_tag=2, stale=stale, bugs=("stale_unconsumed",))
        assert got[(1, 0, 0)] == "fresh"
    with pytest.raises(AssertionError):  # ... and the checker notices when it does not
        for seed in range(10):
            got = sim.run({0: [[("send", 1, 5, "fresh")]], 1: [[("recv", 0, 5)]]}, seed=seed, comm_tag=2, stale=stale,
                          bugs=("stale_unconsumed", "no_clear"))
            assert got[(1, 0, 0)] == "fresh"
    # the protocol before (nothing cleared, the communicator's number in the upper half of the word) kept such a record out by that
    # number -- and the checker notices when it is not looked at
    stale = {(0, 1): [((1 << 32) | (b + 1), 5) for b in range(sim.K)]}
    for seed in range(10):
        got = sim.run({0: [[("send", 1, 5, "fresh")]], 1: [[("recv", 0, 5)]]}, seed=seed, comm_tag=2, stale=stale, bugs=("stale_unconsumed",), protocol="packed")
        assert got[(1, 0, 0)] == "fresh"
    with pytest.raises(AssertionError):
        for seed in range(10):
            got = sim.run({0: [[("send", 1, 5, "fresh")]], 1: [[("recv", 0, 5)]]}, seed=seed, comm_tag=2, stale=stale,
                          bugs=("stale_unconsumed", "no_comm_check"), protocol="packed")
            assert got[(1, 0, 0)] == "fresh"


def _ping(m):
    """m messages 0 -> 1 and their echoes, tags alternating"""
    return {0: [[("send", 1, 40 + (k & 1), f"m{k}") for k in range(m)] + [("recv", 1, 40 + (k & 1)) for k in range(m)]],
            1: [[("recv", 0, 40 + (k & 1)) for k in range(m)] + [("send", 0, 40 + (k & 1), f"e{k}") for k in range(m)]]}


def _check_ping(got, m):
    assert [got[(1, 0, k)] for k in range(m)] == [f"m{k}" for k in range(m)] and [got[(0, 0, m + k)] for k in range(m)] == [f"e{k}" for k in range(m)]


A_TAG, B_TAG = (1 << 32) - 40 + 1, (1 << 32) + 60 + 1  # born at epoch 2^32 - 40; its successor, born at 2^32 + 60


def _left_by(tag32, packed):
    """what a communicator that exchanged 11 messages per pair, all consumed and answered, leaves in every box"""
    last = [11 - (11 - 1 - b) % sim.K for b in range(sim.K)]
    return {pair: [(((tag32 << 32) | n) if packed else n, 41) for n in last] for pair in ((0, 1), (1, 0))}


def test_a_communicator_that_succeeds_one_across_2_to_the_32():
    """B's number is smaller than A's in its low 32 bits.  Before, that left every `taken` word above every message B would ever post (a
    receive that never matches) and every ack above everything B's sends wait for (a send that completes unconsumed): the model reports
    it at those semantics, and nothing with the pages cleared at connect"""
    for seed in range(10):
        _check_ping(sim.run(_ping(12), seed=seed, comm_tag=B_TAG, stale=_left_by(A_TAG & sim.M32, False)), 12)
    seen = set()
    for seed in range(10):
        with pytest.raises(sim.Violation) as e:
            sim.run(_ping(12), seed=seed, comm_tag=B_TAG, stale=_left_by(A_TAG & sim.M32, True), protocol="packed")
        seen.add("deadlock" if "deadlock" in str(e.value) else "early" if "completed before" in str(e.value) else str(e.value))
    assert seen <= {"deadlock", "early"} and "early" in seen, seen  # (the silent one: a Send that says "consumed" to nobody)
    # the other way round -- numbers that grow -- the old protocol was right: the model does not cry wolf
    for seed in range(10):
        _check_ping(sim.run(_ping(12), seed=seed, comm_tag=B_TAG + 100, stale=_left_by(B_TAG & sim.M32, True), protocol="packed"), 12)


def test_message_2_to_the_32_of_a_pair():
    """40 messages from message 2^32 - 15 on.  Before, message 2^32 carried into the communicator's number and its n read 0 -- box 7,
    no wait for the box's ack: reported at those semantics; the 64-bit number passes"""
    s0 = (1 << 32) - 16
    for seed in range(10):
        _check_ping(sim.run(_ping(40), seed=seed, comm_tag=7, seq0=s0), 40)
        with pytest.raises(sim.Violation):
            sim.run(_ping(40), seed=seed, comm_tag=7, seq0=s0, protocol="packed")
    for seed in range(5):  # (far from the edge the old protocol passes with the same seeding)
        _check_ping(sim.run(_ping(40), seed=seed, comm_tag=7, seq0=800, protocol="packed"), 40)


def test_the_checker_notices_a_missing_box_wait():
    """a sender that does not wait for the previous occupant's ack overwrites an unconsumed message once the boxes wrap"""
    ops = {0: [[("send", 1, k, k)] for k in range(12)], 1: [[("recv", 0, k) for k in reversed(range(12))]]}
    bad = 0
    for seed in range(30):
        try:
            sim.run(ops, seed=seed, bugs=("no_box_wait",))
        except sim.Violation:
            bad += 1
    assert bad > 0
