"""XMPI_SUM_WIDE on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc path, the ranks meeting on the
device), then the other layouts at one size each.  Scenarios: tests/wide_scenarios.py, every result held to the numpy restatement of
the operator (tests/wide_ref.py).  What stays with the virtual devices (tests/test_wide_devsim.py): ranks in different calls -- an
error path, run where nothing can wedge a GPU.  (The refusal of a stepped name is decided before any launch: it runs here too.)"""
import pytest

from tests.wide_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 8]


@pytest.mark.parametrize("size", SIZES)
def test_every_algorithm_name_at_every_count(size):
    run_ranks("names", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size):
    outs = run_ranks("forms", size, timeout=240)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_and_iallreduce(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_on_other_types_it_is_the_plain_sum_and_the_same_call(size):
    run_ranks("other_types", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_table_row_naming_a_stepped_schedule_runs_the_fold(size):
    run_ranks("table", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_stepped_name_is_refused_on_every_rank(size):
    run_ranks("refused", size, timeout=240)


def test_rank_threads_in_one_process():
    run_threads("layout", 4, {"expect_host_fold": 1}, timeout=240)


def test_ranks_that_meet_on_the_host():
    run_ranks("layout", 3, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


def test_staged_tables():
    run_ranks("layout", 3, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})
