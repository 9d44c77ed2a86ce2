"""xmpi_reduce_scatter and xmpi_alltoall on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc path, the
ranks meeting on the device), then the other layouts.  Scenarios: tests/personal_scenarios.py, every result held to the oracle bit
for bit.  What stays with the virtual devices (tests/test_personal_devsim.py): ranks in different calls -- an error path, run where
nothing can wedge a GPU -- and 9 / 12 ranks, which on ONE GPU would be more processes than it schedules at once."""
import pytest

from tests.personal_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", [2, 3, 4, 8])
def test_every_algorithm_name(size):
    run_ranks("algos", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 4, 8])
def test_every_dtype_and_operation_at_every_count(size):
    run_ranks("sweep", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 4, 8])
def test_host_slices_unregistered_memory_and_streams(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 4, 8])
def test_a_captured_graph_replayed(size):
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_slot_parity_across_kinds_of_collective(size):
    run_ranks("parity", size, timeout=240)


@pytest.mark.parametrize("size", [2, 4])
def test_rank_threads_in_one_process(size):
    run_threads("layout", size, {"expect_host_fold": 1}, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_ranks_that_meet_on_the_host(size):
    run_ranks("layout", size, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", [2, 3, 8])
def test_staged_tables(size):
    run_ranks("layout", size, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


@pytest.mark.parametrize("size", [2, 3, 8])
def test_reduce_scatter_on_hard_floats(size):
    """reduce-scatter's rank-order fold where it can be seen -- dense mantissas, NaNs, infinities, signed zeros, subnormals
    (tests/hard_inputs.py) -- by every name, one kernel and meet / body / done; all-to-all of the same data byte for byte"""
    run_ranks("hard", size, timeout=240)


def test_hard_floats_in_the_other_layouts():
    """the host rendezvous (XMPI_DSYNC=0, and rank threads of one process) and the staged tables (XMPI_ZERO_COPY=0 as well)"""
    run_ranks("hard", 3, {"expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})
    run_ranks("hard", 3, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})
    run_threads("hard", 2, timeout=240)


def test_full_size():
    """8 ranks x 32 MiB per block, f32: the whole buffers compared on the device with an uploaded expectation"""
    run_ranks("fullsize", 8, timeout=300)
