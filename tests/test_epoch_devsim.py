"""The device counters across their 32-bit edges, on virtual devices (tests/devsim, one process per device; see tests/test_devsim.py):
the epoch the kernels count, the communicator's number and the message number of an ordered pair, started next to an edge by the
test-only variables XMPI_TEST_EPOCH_BASE and XMPI_TEST_P2P_SEQ0.  Scenarios: tests/epoch_scenarios.py, every result compared bit for
bit with the oracle.  Every job has XMPI_TIMEOUT_S of a few seconds: a wait that never matches is an XMPI_ERR_TIMEOUT in the rank's
output, not a hang.  No GPU involved."""
import json
import os
import re
import uuid

import pytest

from tests.epoch_harness import SEQ0, env, run_ranks

SIZES = [2, 3, 8]
BASES = [2 ** 31 - 24, 2 ** 32 - 24, 2 ** 32 - 1, 3 * 2 ** 32 - 24, 2 ** 40 - 24]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epoch_unset_parent.json")


@pytest.fixture(scope="module", autouse=True)
def devsim_lib():
    from tests.devsim import build
    path = build.build_lib()
    old = os.environ.get("XMPI_DEVSIM_LIB")
    os.environ["XMPI_DEVSIM_LIB"] = path  # (the harness hands the environment on to the rank processes)
    yield path
    if old is None:
        del os.environ["XMPI_DEVSIM_LIB"]
    else:
        os.environ["XMPI_DEVSIM_LIB"] = old


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("size", SIZES)
def test_every_form_across_the_edge(size, base):
    """what fits of every form below the edge, a captured graph of LL collectives replayed onto the edge itself (epochs k 2^32 and
    k 2^32 + 1: the same flag, the other parity), every form, the agent's runs and a ring of Send / Receive above it"""
    outs = run_ranks("cross", size, {"base": base}, timeout=240, env=env(base))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("base", [2 ** 32 - 24, 2 ** 32 - 1])
@pytest.mark.parametrize("size", SIZES)
def test_the_agent_counts_across_the_edge(size, base):
    """... with the agent's consecutive blocking calls (prev_epoch + 1, the page not read) on the edge instead of the graph"""
    outs = run_ranks("cross", size, {"base": base, "edge_by": "agent"}, timeout=240, env=env(base))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("base", [2 ** 32 - 40, 5 * 2 ** 32 - 40])
@pytest.mark.parametrize("size", SIZES)
def test_a_communicator_that_succeeds_one_across_the_edge(size, base):
    """A is born below the edge and leaves its pooled pages full of its numbers; B takes the same pages, born above the edge: its
    number is smaller than A's in the low 32 bits.  Its Sends must wait for their Receives, its Receives must find their messages"""
    outs = run_ranks("succession", size, {"base": base, "key": uuid.uuid4().hex[:8]}, timeout=240, env=env(base))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_message_2_to_the_32_of_every_pair(size):
    """40 messages per ordered pair from message 2^32 - 15 on: tags alternate, every payload, length and tag is checked"""
    outs = run_ranks("message_wrap", size, timeout=240, env=env(seq0=SEQ0))
    assert "messages checked" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_message_2_to_the_32_in_a_succeeding_communicator(size):
    outs = run_ranks("succession", size, {"base": 2 ** 32 - 40, "key": uuid.uuid4().hex[:8], "wrap": 1}, timeout=240, env=env(2 ** 32 - 40, SEQ0))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_both_variables_unset_change_nothing(size):
    """a fixed sequence of every form: the launch counters and the epoch afterwards are what the commit before the two variables gave
    (tests/golden/epoch_unset_parent.json, recorded there by running this scenario against that commit's library)"""
    outs = run_ranks("unset", size, timeout=240, env=env())
    got = dict(re.findall(r"(\w+)=(-?\d+)", [ln for ln in outs[0].splitlines() if ln.startswith("epoch unset counters:")][0]))
    with open(GOLDEN) as f:
        want = json.load(f)[str(size)]
    assert {k: int(v) for k, v in got.items()} == want
