"""The device counters across their 32-bit edges on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc
path, the ranks meeting on the device).  Scenarios: tests/epoch_scenarios.py, every result compared bit for bit with the oracle; the
same scenarios run at every base and size on the virtual devices first (tests/test_epoch_devsim.py).  Every job has XMPI_TIMEOUT_S
of a few seconds -- a wait that never matches ends its kernel with XMPI_ERR_TIMEOUT -- and runs in child processes
(tests/epoch_worker.py) under the harness's own time limit: the test runner itself never opens the GPU."""
import uuid

import pytest

from tests.epoch_harness import SEQ0, env, run_ranks

pytestmark = pytest.mark.gpu


def _args(size, **kw):
    """8 processes share ONE GPU here and take turns on it, so the job of 8 runs the covering subset: one call of each form above
    the edge (tests/epoch_scenarios.py sc_cross); the whole sequence runs with 2 and 3 processes here and at every size on the
    virtual devices"""
    return dict(kw, cover=1) if size == 8 else kw


@pytest.mark.parametrize("base", [2 ** 32 - 24, 2 ** 32 - 1])
@pytest.mark.parametrize("size", [2, 3, 8])
def test_every_form_across_the_edge(size, base):
    outs = run_ranks("cross", size, _args(size, base=base), timeout=120, env=env(base))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("size", [2, 3])
def test_the_agent_counts_across_the_edge(size):
    outs = run_ranks("cross", size, {"base": 2 ** 32 - 24, "edge_by": "agent"}, timeout=120, env=env(2 ** 32 - 24))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("base", [2 ** 32 - 40, 5 * 2 ** 32 - 40])
@pytest.mark.parametrize("size", [2, 3])
def test_a_communicator_that_succeeds_one_across_the_edge(size, base):
    outs = run_ranks("succession", size, {"base": base, "key": uuid.uuid4().hex[:8]}, timeout=120, env=env(base))
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("size", [2, 3])
def test_message_2_to_the_32_of_every_pair(size):
    outs = run_ranks("message_wrap", size, timeout=120, env=env(seq0=SEQ0))
    assert "messages checked" in outs[0]


@pytest.mark.parametrize("size", [2, 3])
def test_message_2_to_the_32_in_a_succeeding_communicator(size):
    outs = run_ranks("succession", size, {"base": 2 ** 32 - 40, "key": uuid.uuid4().hex[:8], "wrap": 1}, timeout=120, env=env(2 ** 32 - 40, SEQ0))
    assert "calls checked" in outs[0]
