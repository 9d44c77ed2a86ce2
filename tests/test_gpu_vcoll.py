"""xmpi_alltoallv on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc path, the ranks meeting on
the device, the counts read and exchanged by the kernels), then the layouts whose ranks meet on the host.  Scenarios:
tests/vcoll_scenarios.py, every result compared whole, byte for byte.  What stays with the virtual devices
(tests/test_vcoll_devsim.py): the error paths -- run where nothing can wedge a GPU -- and 9 / 12 ranks."""
import pytest

from tests.vcoll_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu
HOST = {"expect_host": 1, "expect_params": {"dsync": 0}}


@pytest.mark.parametrize("size", [2, 3, 8])
def test_every_layout_dtype_and_algorithm_name(size):
    """packed, slotted with gaps, odd base, residues that differ, skewed -- U8, F16, I64 by AUTO / ZCOPY / DIRECT; dsync_v_launches
    says which path ran"""
    run_ranks("layouts", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_equal_counts_give_what_alltoall_gives(size):
    run_ranks("equal", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_host_slices_unregistered_memory_and_the_stream_form(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_a_captured_graph_replays_with_new_counts(size):
    """captured once (a single chain on one stream), replayed 3 times with a different count matrix in the device arrays"""
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_forty_calls_back_to_back_between_other_collectives(size):
    run_ranks("back_to_back", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_ranks_that_meet_on_the_host(size):
    run_ranks("layouts", size, HOST, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", [2, 4])
def test_rank_threads_in_one_process(size):
    run_threads("layouts", size, {"expect_host": 1}, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_without_zero_copy(size):
    run_ranks("layouts", size, {"expect_host": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})
